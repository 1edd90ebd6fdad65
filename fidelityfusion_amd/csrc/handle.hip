// libffgp handle: life cycle and streams, workspace, options, stage timing.  See include/ffgp.h.
#include <atomic>
#include <iterator>
#include <cmath>
#include <strings.h>

#include "drivers.h"

#define SCAL_DOUBLES 2048

static const char* k_stage_names[FFGP_MAX_STAGES] = {"assemble", "potrf", "reduce", "trtri", "lauum", "grad",
                                                     "predict_gemm", "", "", "", "", "", "", "", "", ""};

int ffgp_ensure_ws(ffgp_handle* h, size_t bytes) {
  if (bytes <= h->ws_bytes) return FFGP_OK;
  if (h->ws) {
    hipStreamSynchronize(h->stream);
    hipFree(h->ws);
    h->ws = nullptr;
    h->ws_bytes = 0;
  }
  // round up to 64 MiB so a slowly growing problem does not reallocate on every call
  const size_t gran = (size_t)64 << 20;
  const size_t want = (bytes + gran - 1) / gran * gran;
  if (hipMalloc(&h->ws, want) != hipSuccess) {
    fprintf(stderr, "[ffgp] workspace allocation of %zu bytes failed\n", want);
    (void)hipGetLastError();   // (the failed hipMalloc's sticky status must not fail the next, smaller, call's launch checks)
    h->ws = nullptr;
    return FFGP_ERR_ALLOC;
  }
  h->ws_bytes = want;
  ++h->alloc_epoch;
  return FFGP_OK;
}

__global__ void ffgp_zero_words(unsigned* __restrict__ p, size_t nwords) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

int ffgp_zero_async(ffgp_handle* h, void* ptr, size_t bytes) {
  if (!bytes) return FFGP_OK;
  if (bytes > ((size_t)8 << 20) || (bytes & 3)) {
    FFGP_HIP(hipMemsetAsync(ptr, 0, bytes, h->stream));
    return FFGP_OK;
  }
  const size_t nw = bytes >> 2;
  const unsigned grid = (unsigned)((nw + 255) / 256 < 2048 ? (nw + 255) / 256 : 2048);
  hipLaunchKernelGGL(ffgp_zero_words, dim3(grid), dim3(256), 0, h->stream, (unsigned*)ptr, nw);
  return FFGP_OK;
}

void stage_mark(ffgp_handle* h, int idx) {
  if (h->timing >= 1 && idx <= FFGP_MAX_STAGES) {
    hipEventRecord(h->ev[idx], h->stream);
    if (idx > h->n_stages) h->n_stages = idx;
  }
}

void stage_collect(ffgp_handle* h) {
  if (h->timing < 1) return;
  for (int i = 0; i < FFGP_MAX_STAGES; ++i) h->stage_ms[i] = 0.f;
  for (int i = 0; i < h->n_stages; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]) == hipSuccess) h->stage_ms[i] = ms;
  }
}

void ffgp_rawg_drop(RawGraph* r) {
  if (!r) return;
  if (r->valid) {
    hipGraphExecDestroy(r->exec);
    hipGraphDestroy(r->graph);
  }
  r->valid = false;
  r->seen = 0;
}

extern "C" {

const char* ffgp_version(void) { return "ffgp 0.6 (gfx950, fp64 MFMA)"; }
int ffgp_has_dev_options(void) { return 0; }   // (always 0: kept for existing bindings)

long ffgp_graph_replays(const ffgp_handle* h) { return h ? h->graph_replays : -1; }

static int create_resources(ffgp_handle* h) {
  FFGP_HIP(hipStreamCreate(&h->stream));
  h->own_stream = true;
  h->own = h->stream;
  int lo = 0, hi = 0;  // numerically lowest value = greatest priority
  FFGP_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
  FFGP_HIP(hipStreamCreateWithPriority(&h->aux, hipStreamNonBlocking, hi));
  // the look-ahead hand-offs order kernels of ONE device (their dispatch packets carry the agent-scope release / acquire): no
  // system-scope fence at record time -- N = 4096 2.00 -> 1.97 ms, N = 8192 5.87 -> 5.83 (FFGP_EVFLAGS overrides: development)
  const unsigned evflags = getenv("FFGP_EVFLAGS") ? (unsigned)strtoul(getenv("FFGP_EVFLAGS"), nullptr, 0) : (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
  for (int i = 0; i < 10; ++i) FFGP_HIP(hipEventCreateWithFlags(&h->la_ev[i], evflags));
  FFGP_HIP(hipMalloc(&h->d_info, 16 * sizeof(int)));
  FFGP_HIP(hipMemset(h->d_info, 0, 16 * sizeof(int)));
  FFGP_HIP(hipMalloc(&h->ho_mem, 10 * 16 * sizeof(unsigned)));
  FFGP_HIP(hipMemset(h->ho_mem, 0, 10 * 16 * sizeof(unsigned)));
  h->ho_selftest_pending = 1;      // (the value operations are tried once on the side stream, below, after the NULL-stream memsets are visible)
  FFGP_HIP(hipDeviceSynchronize());   // NULL-stream memset: make it visible before any (non-blocking) stream touches it
  if (h->ho_values && h->ho_selftest_pending) {
    // a runtime / driver without the stream value operations keeps the event pairs: one write + wait on an unused word of the hand-off store
    h->ho_selftest_pending = 0;
    unsigned* probe = h->ho_mem + 15;
    const bool ok = hipStreamWriteValue32(h->aux, probe, 1u, 0) == hipSuccess &&
                    hipStreamWaitValue32(h->aux, probe, 1u, hipStreamWaitValueGte, 0xffffffffu) == hipSuccess &&
                    hipStreamSynchronize(h->aux) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      h->ho_values = 0;
    }
  }
  if (h->ho_values && h->own) {      // ... and a wait enqueued BEFORE its producer on another stream must come through (potrf.hip)
    const int st = ffgp_handoff_selftest(h);
    if (st != 0) {
      if (st < 0) (void)hipGetLastError();
      h->ho_values = 0;
      h->ho_selftest_failed = 1;
    }
  }
  FFGP_HIP(hipMalloc(&h->d_scal, SCAL_DOUBLES * sizeof(double)));
  FFGP_HIP(hipHostMalloc(&h->h_info, 16 * sizeof(int)));
  memset(h->h_info, 0, 16 * sizeof(int));
  FFGP_HIP(hipHostMalloc(&h->h_scal, 64 * sizeof(double)));
  for (int i = 0; i <= FFGP_MAX_STAGES; ++i) FFGP_HIP(hipEventCreate(&h->ev[i]));
  FFGP_HIP(hipEventCreate(&h->syrk_ev[0]));
  FFGP_HIP(hipEventCreate(&h->syrk_ev[1]));
  return FFGP_OK;
}

int ffgp_ensure_aux2(ffgp_handle* h) {
  if (h->aux2) return FFGP_OK;
  FFGP_HIP(hipStreamCreateWithFlags(&h->aux2, hipStreamNonBlocking));
  FFGP_HIP(hipStreamCreateWithFlags(&h->aux3, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) FFGP_HIP(hipEventCreateWithFlags(&h->tri_ev[i], hipEventDisableTiming));
  return FFGP_OK;
}

// ROCm binds a stream to one of its hardware queues at the stream's first USE, streams on one queue run in order, and a stream that
// first appears late shares a queue with whatever is least loaded then.  The handle's third stream (head of the triangular inverse under
// the factorisation's tail) is created by the first training step of a large block -- in a process that had reserved worker streams
// before, it landed on the caller's queue and the head ran in line with the trailing updates instead of beside them (N = 4096 training
// step 3.12 -> 3.40-3.49 ms with GPU_MAX_HW_QUEUES = 6, tools/queue_probe.py).  A process that is going to put several blocks in flight
// calls this for its main handle BEFORE it creates the worker streams (fidelityfusion_amd._lib.configure_queues does).
extern "C" int ffgp_prepare_streams(ffgp_handle* h) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_CHECK(ffgp_ensure_aux2(h));
  FFGP_HIP(hipMemsetAsync(h->d_info + 8, 0, sizeof(int), h->aux));
  FFGP_HIP(hipMemsetAsync(h->d_info + 9, 0, sizeof(int), h->aux2));
  FFGP_HIP(hipMemsetAsync(h->d_info + 10, 0, sizeof(int), h->aux3));
  FFGP_HIP(hipStreamSynchronize(h->aux));
  FFGP_HIP(hipStreamSynchronize(h->aux2));
  FFGP_HIP(hipStreamSynchronize(h->aux3));
  return FFGP_OK;
}

// Value hand-offs (potrf.hip) make a stream WAIT inside a one-workgroup kernel for a word another queue's kernel will write.  Anything
// that runs the process's kernels strictly one at a time -- rocprofv3's counter collection (--pmc / counter groups: it serialises the
// dispatches of all queues; seen as a hang of the PMC passes of tools/profile_round.sh), thread trace, the rocprofiler v1 / v2 tools,
// HIP_LAUNCH_BLOCKING, AMD_SERIALIZE_KERNEL -- would leave that kernel spinning for a producer that can never start.  In such a
// process the handle keeps the event pairs (the command processor waits for those, no kernel does).  FFGP_HANDOFF=events / values
// overrides the detection.
// handles alive in this process (ffgp_live_handles): a lone handle may assume the chip is its own between its kernels
static std::atomic<int> g_live_handles{0};
extern "C++" int ffgp_live_handles() { return g_live_handles.load(std::memory_order_relaxed); }

static bool env_on(const char* key) {
  const char* v = getenv(key);
  return v && *v && strcmp(v, "0") && strcasecmp(v, "false") && strcasecmp(v, "off");
}
static int default_ho_values() {
  const char* f = getenv("FFGP_HANDOFF");
  if (f && !strcmp(f, "events")) return 0;
  if (f && !strcmp(f, "values")) return 1;
  static const char* const serialising[] = {"ROCPROF_COUNTER_COLLECTION", "ROCPROF_COUNTERS", "ROCPROF_COUNTER_GROUPS", "ROCPROF_ADVANCED_THREAD_TRACE",
                                            "ROCP_METRICS", "ROCPROFILER_METRICS_PATH", "HIP_LAUNCH_BLOCKING", "CUDA_LAUNCH_BLOCKING",
                                            "AMD_SERIALIZE_KERNEL", "AMD_SERIALIZE_COPY"};
  for (const char* k : serialising)
    if (env_on(k)) return 0;
  const char* tools = getenv("HSA_TOOLS_LIB");
  if (tools && (strstr(tools, "rocprofiler64") || strstr(tools, "libroctracer"))) return 0;
  return 1;
}

int ffgp_create(int device, ffgp_handle** out) {
  if (!out) return FFGP_ERR_ARG;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
    fprintf(stderr, "[ffgp] no usable HIP device (requested %d of %d); libffgp has no CPU fallback\n", device, count);
    return FFGP_ERR_NODEVICE;
  }
  FFGP_HIP(hipSetDevice(device));
  ffgp_handle* h = new ffgp_handle();  // value-initialised: every POD member is zero
  h->device = device;
  h->lookahead = 1;
  h->small_tile_threshold = 640;
  h->batch_grad_ob = 1;
  h->tile32_threshold = 1024;
  h->polite_m = 8192;
  h->split_rem_max = 180;
  h->syrk_light_tiles = 1;
  h->super_block = 1024;
  h->splitk_min_k = 1024;
  h->tlin_gemm_min = 8192;      // (profiles/train_tlin_bench.txt: the plain kernels win up to n l h = 2048, the GEMM from 14400 on)
  h->skinny_max_n = 8;
  h->super_min_n = 2048;
  h->la_carry = 2;
  h->la_carry_n = 12288;
  h->la_carry_rows = 8192;
  h->la_min_n = 1024;
  h->chase_xl = 1;
  h->chase_xl_max_n = 2048;
  {   // (handles of one process prefer different XCDs: blocks in flight from several host threads do not crowd one)
    static std::atomic<int> next_xcc{0};
    h->chase_xcc = next_xcc.fetch_add(1) & 7;
  }
  h->aux_prio = 1;
  h->nb_outer = 512;
  h->trsm128 = 1;
  h->polite64_pad_kb = 60;
  h->polite32_pad_kb = 46;
  h->ho_values = default_ho_values();
  h->ho_defer = 2;
  h->ho_gate = 1;
  h->grad_lanes = 3;
  h->ho_timeout_ms = 2000;
  h->ho_defer_slot = -1;
  h->ho_gdefer_slot = -1;
  h->diag_excl_rows = 4096;
  h->trsm128_max_m = 8192;
  h->trtri_overlap = 1;
  h->small2_off = 1;
  h->q2_split_min_cols = 8192;
  h->sb_lower = 1;
  h->sb_lower_min_n = 6144;
  h->sb_sym_wg = 2048;
  h->asm_mm = 1;
  h->asm_mm_min = 6144;
  h->asm_mm_grid = 768;
  const int rc = create_resources(h);
  if (rc != FFGP_OK) {   // release whatever was created before the failure
    ffgp_destroy(h);
    return rc;
  }
  g_live_handles.fetch_add(1, std::memory_order_relaxed);
  h->counted_live = 1;
  *out = h;
  return FFGP_OK;
}

int ffgp_destroy(ffgp_handle* h) {
  if (!h) return FFGP_OK;
  if (h->counted_live) {
    g_live_handles.fetch_sub(1, std::memory_order_relaxed);
    h->counted_live = 0;
  }
  hipSetDevice(h->device);
  if (h->own) hipStreamSynchronize(h->own);
  if (h->aux) hipStreamSynchronize(h->aux);
  if (h->ws) hipFree(h->ws);
  if (h->dinv) hipFree(h->dinv);
  if (h->sinv) hipFree(h->sinv);
  if (h->tsw) hipFree(h->tsw);
  if (h->skw) hipFree(h->skw);
  if (h->ews) hipFree(h->ews);
  if (h->d_link) hipFree(h->d_link);
  if (h->aux2) hipStreamDestroy(h->aux2);
  if (h->aux3) hipStreamDestroy(h->aux3);
  if (h->ev_switch) hipEventDestroy(h->ev_switch);
  for (int i = 0; i < 2; ++i)
    if (h->tri_ev[i]) hipEventDestroy(h->tri_ev[i]);
  if (h->d_info) hipFree(h->d_info);
  if (h->ho_mem) hipFree(h->ho_mem);
  if (h->bt_info) hipFree(h->bt_info);
  if (h->train_g) hipFree(h->train_g);
  if (h->train_tree) hipFree(h->train_tree);
  for (int z = 0; z < FFGP_GRAD_LANES; ++z) {
    if (h->lane_ev[z]) hipEventDestroy(h->lane_ev[z]);
    if (z > 0 && h->lane_skw[z]) hipFree(h->lane_skw[z]);
  }
  if (h->lane_scal) hipFree(h->lane_scal);
  if (h->small_kbuf) hipFree(h->small_kbuf);
  if (h->train_blk) hipFree(h->train_blk);
  if (h->train_blk_host) hipHostFree(h->train_blk_host);
  ffgp_assemble_collect_free(h);
  if (h->bt_info_host) hipHostFree(h->bt_info_host);
  if (h->d_scal) hipFree(h->d_scal);
  if (h->d_asm) hipFree(h->d_asm);
  ffgp_rawg_drop(h->fwdg);
  if (h->fwdg) {
    if (h->fwdg->stage) hipFree(h->fwdg->stage);
    delete h->fwdg;
    h->fwdg = nullptr;
  }
  if (h->h_info) hipHostFree(h->h_info);
  if (h->h_scal) hipHostFree(h->h_scal);
  for (int i = 0; i <= FFGP_MAX_STAGES; ++i)
    if (h->ev[i]) hipEventDestroy(h->ev[i]);
  for (int i = 0; i < 2; ++i)
    if (h->syrk_ev[i]) hipEventDestroy(h->syrk_ev[i]);
  for (hipEvent_t e : h->syrk_pool) hipEventDestroy(e);
  for (int i = 0; i < 10; ++i)
    if (h->la_ev[i]) hipEventDestroy(h->la_ev[i]);
  if (h->aux) hipStreamDestroy(h->aux);
  if (h->own) hipStreamDestroy(h->own);
  delete h;
  return FFGP_OK;
}

int ffgp_set_stream(ffgp_handle* h, void* s) {
  if (!h) return FFGP_ERR_ARG;
  hipStream_t ns = s ? reinterpret_cast<hipStream_t>(s) : h->own;
  if (ns == h->stream) return FFGP_OK;
  // Work enqueued through this handle on the stream it leaves may still be running on the handle's workspaces (the asynchronous
  // entry points return before it has): the stream it moves to waits for that work.  Costs nothing while the stream stays the same.
  FFGP_HIP(hipSetDevice(h->device));
  if (!h->ev_switch) FFGP_HIP(hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
  if (hipEventRecord(h->ev_switch, h->stream) == hipSuccess) {
    FFGP_HIP(hipStreamWaitEvent(ns, h->ev_switch, 0));
  } else {
    (void)hipGetLastError();   // (the old stream no longer exists: nothing of it can be running)
  }
  h->stream = ns;
  return FFGP_OK;
}

// ---- options.  Nearly every key is "optional range check, store into one handle field": those live in a table.
enum { OPT_INT, OPT_BOOL, OPT_NOT };      // (int)value | value != 0 | value == 0 (the key switches a path ON, the field says OFF)
struct ffgp_option {
  const char* key;
  int ffgp_handle::*field;
  int kind;
  double lo = -INFINITY, hi = INFINITY;      // values below lo / above hi are refused (a NaN is below and above nothing)
};
static const ffgp_option k_options[] = {
    {"timing", &ffgp_handle::timing, OPT_INT},
    {"naive", &ffgp_handle::use_naive, OPT_INT},
    {"aux_prio", &ffgp_handle::aux_prio, OPT_INT},
    {"batch_grad_ob", &ffgp_handle::batch_grad_ob, OPT_BOOL},
    {"small_tile_threshold", &ffgp_handle::small_tile_threshold, OPT_INT},
    {"tile32_threshold", &ffgp_handle::tile32_threshold, OPT_INT},
    {"fwd_graph", &ffgp_handle::fwd_graph, OPT_BOOL},
    {"ho_gate", &ffgp_handle::ho_gate, OPT_BOOL},
    {"ho_timeout_ms", &ffgp_handle::ho_timeout_ms, OPT_INT, 1.0, 600000.0},
    {"ho_withhold", &ffgp_handle::ho_withhold, OPT_INT},
    {"diag_excl_rows", &ffgp_handle::diag_excl_rows, OPT_INT},
    {"ho_defer", &ffgp_handle::ho_defer, OPT_INT, 0.0, 2.0},
    {"polite32_pad_kb", &ffgp_handle::polite32_pad_kb, OPT_INT, 0.0, 64.0},
    {"polite64_pad_kb", &ffgp_handle::polite64_pad_kb, OPT_INT, 0.0, 64.0},
    {"trsm128", &ffgp_handle::trsm128, OPT_BOOL},
    {"trsm128_max_m", &ffgp_handle::trsm128_max_m, OPT_INT},
    {"la_min_n", &ffgp_handle::la_min_n, OPT_INT},
    {"chase_xl", &ffgp_handle::chase_xl, OPT_INT},
    {"chase_xl_max_n", &ffgp_handle::chase_xl_max_n, OPT_INT},
    {"grad_lanes", &ffgp_handle::grad_lanes, OPT_INT, 1.0, 3.0},
    {"train_persist", &ffgp_handle::train_persist_off, OPT_NOT},
    {"tlin_gemm_min", &ffgp_handle::tlin_gemm_min, OPT_INT, 0.0, 2147483647.0},
    {"chase_xcc", &ffgp_handle::chase_xcc, OPT_INT, 0.0, 15.0},
    {"la_carry", &ffgp_handle::la_carry, OPT_INT},
    {"la_carry_n", &ffgp_handle::la_carry_n, OPT_INT, 0.0},
    {"la_carry_rows", &ffgp_handle::la_carry_rows, OPT_INT, 0.0},
    {"lookahead", &ffgp_handle::lookahead, OPT_INT},
    {"polite_m", &ffgp_handle::polite_m, OPT_INT},
    {"split_rem_max", &ffgp_handle::split_rem_max, OPT_INT},
    {"syrk_light_tiles", &ffgp_handle::syrk_light_tiles, OPT_BOOL},
    {"asm_mm", &ffgp_handle::asm_mm, OPT_INT},
    {"asm_mm_grid", &ffgp_handle::asm_mm_grid, OPT_INT, 1.0},
    {"asm_mm_min", &ffgp_handle::asm_mm_min, OPT_INT},
    {"trtri_fill", &ffgp_handle::trtri_fill, OPT_INT},
    {"trtri_overlap", &ffgp_handle::trtri_overlap, OPT_INT},
    {"small_max_n", &ffgp_handle::small_max_n, OPT_INT},
    {"sb_lower", &ffgp_handle::sb_lower, OPT_BOOL},
    {"sb_lower_min_n", &ffgp_handle::sb_lower_min_n, OPT_INT, 0.0},
    {"sb_sym_wg", &ffgp_handle::sb_sym_wg, OPT_INT, 64.0, 65536.0},
    {"q2_split_min_cols", &ffgp_handle::q2_split_min_cols, OPT_INT},
    {"small_finish", &ffgp_handle::small2_off, OPT_NOT},
    {"small_fused", &ffgp_handle::small_off, OPT_NOT},
    {"chase_pack", &ffgp_handle::chase_pack, OPT_INT},
    {"skinny_max_n", &ffgp_handle::skinny_max_n, OPT_INT},
    {"splitk_min_k", &ffgp_handle::splitk_min_k, OPT_INT},
    {"super_min_n", &ffgp_handle::super_min_n, OPT_INT},
};

int ffgp_set_option(ffgp_handle* h, const char* key, double value) {
  if (!h || !key) return FFGP_ERR_ARG;
  ffgp_rawg_drop(h->fwdg);      // a captured call baked the old options in
  // the keys whose rule is not a range
  if (!strcmp(key, "nb_outer")) {
    const int v = (int)value;
    if (v < FFGP_NB || v % FFGP_NB) return FFGP_ERR_ARG;
    h->nb_outer = v;
  } else if (!strcmp(key, "gemm_tile")) {
    const int v = (int)value;
    if (v != 0 && v != 32 && v != 64 && v != 128) return FFGP_ERR_ARG;
    h->force_ts = v;
  } else if (!strcmp(key, "super_block")) {
    const int v = (int)value;
    if (v != 0 && (v < 2 * FFGP_NB || (v & (v - 1)))) return FFGP_ERR_ARG;   // 0, or a power of two >= 256
    h->super_block = v;
    h->sinv_L = nullptr;
  } else if (!strcmp(key, "ho_values")) {
    if (value != 0.0 && h->ho_selftest_failed) return FFGP_ERR_ARG;      // (this process runs its kernels one at a time: see ffgp_handoff_selftest)
    h->ho_values = value != 0.0;
  } else {
    const ffgp_option* o = k_options;
    while (o != std::end(k_options) && strcmp(key, o->key)) ++o;
    // (the switches of experiments that were measured and lost, docs/experiments.md, are gone: their keys are refused like any unknown key)
    if (o == std::end(k_options) || value < o->lo || value > o->hi) return FFGP_ERR_ARG;
    h->*o->field = (o->kind == OPT_INT) ? (int)value : (o->kind == OPT_BOOL) ? (value != 0.0 ? 1 : 0) : (value == 0.0 ? 1 : 0);
  }
  return FFGP_OK;
}

// ---- instrumentation
int ffgp_last_timings(ffgp_handle* h, float* ms_out, const char** names_out, int max_stages, int* n_stages) {
  if (!h || !ms_out || !n_stages) return FFGP_ERR_ARG;
  const int ns = h->n_stages < max_stages ? h->n_stages : max_stages;
  for (int i = 0; i < ns; ++i) {
    ms_out[i] = h->stage_ms[i];
    if (names_out) names_out[i] = k_stage_names[i];
  }
  *n_stages = ns;
  return FFGP_OK;
}

int ffgp_syrk_stats(ffgp_handle* h, double* flops, double* ms, long* launches, int reset) {
  if (!h) return FFGP_ERR_ARG;
  if (h->syrk_pool_used > 0) {
    hipSetDevice(h->device);
    hipEventSynchronize(h->syrk_pool[h->syrk_pool_used - 1]);
    for (int i = 0; i + 1 < h->syrk_pool_used; i += 2) {
      float ms_i = 0.f;
      if (hipEventElapsedTime(&ms_i, h->syrk_pool[i], h->syrk_pool[i + 1]) == hipSuccess) h->syrk_ms += ms_i;
    }
    h->syrk_pool_used = 0;
  }
  if (flops) *flops = h->syrk_flops;
  if (ms) *ms = h->syrk_ms;
  if (launches) *launches = h->syrk_launches;
  if (reset) {
    h->syrk_flops = 0.0;
    h->syrk_ms = 0.0;
    h->syrk_launches = 0;
  }
  return FFGP_OK;
}

}  // extern "C"

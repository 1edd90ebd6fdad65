// libffgp C ABI: handle lifetime, workspace, fused NLML (+ gradients) and posterior paths.  See include/ffgp.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <strings.h>

#include "ffgp_internal.h"

int ffgp_assemble_impl(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                       const double* amp, double clamp_min, const double* diag_add, const double* diag_vec,
                       long diag_stride, const double* add_mat, int ld_add, double add_all, double mean_jitter, double* K,
                       int ldk, int lower_only, int kfun, double kparam);
int ffgp_transpose(ffgp_handle* h, const double* src, int rows, int cols, int ld_src, double* dst, int ld_dst, double scale);
int ffgp_trtri_impl(ffgp_handle* h, const double* L, int n, int ldl, double* X, int ldx, double* T);
int ffgp_lauum_impl(ffgp_handle* h, const double* X, int n, int ldx, double* S, int lds_);
int ffgp_trtri_lauum_ob(ffgp_handle* h, int F, const double* L0, long sL, int n, int ldl, double* X0, long sX, int ldx, double* T0, long sT,
                        double* S0, long sS, int lds_, const double* dinv0, long sD);
int ffgp_nll_reduce_impl(ffgp_handle* h, int variant, const double* L, int n, int ldl, const double* M, int rows, int cols,
                         int ldm, int d, double pi_const, double* out_dev);
int ffgp_grad_impl(ffgp_handle* h, const double* X, int n, int D, const double* w, const double* amp, double clamp,
                   const double* G, int ldg, double mean_jitter, double* g_w, double* g_amp, double* g_diag_add,
                   double* g_diag_vec, double* partial_ws, int kfun, double kparam, double* g_kparam);
size_t ffgp_grad_partial_doubles(int n, int D);
int ffgp_kernel_grad_impl(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                          const double* amp, double clamp, int kfun, double kparam, const double* dK, int ldk, double* g_w,
                          double* g_amp, double* g_kparam);
int ffgp_kernel_wt_impl(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                        const double* amp, double clamp, int kfun, double kparam, const double* dK, int ldk, double* Wt,
                        int ldw);

int ffgp_assemble_pair_impl(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                            const double* diag_add, const double* diag_vec, long diag_stride, const double* add_mat, int ld_add,
                            double add_all, double mean_jitter, double* K, int ldk, int lower_only);
size_t ffgp_grad_pair_partial_doubles(int n1, int n2, int D, int rect, int nl);
int ffgp_grad_pair_impl(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                        const double* G, int ldg, int rect, const double* trG_dev, double mj_coef, double* partial_ws,
                        const ffgp_kdesc_grads* g);
int ffgp_pair_wt_impl(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t, const double* dK,
                      int ldk, double* Wt, int ldw, long leaf_stride);
int ffgp_rows_in_impl(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, unsigned char* found);

int ffgp_syevj_small_impl(ffgp_handle* h, const double* M, int n, int ldm, int batch, long strideM, double* Q, int ldq,
                          long strideQ, double* evals, long strideE, int descending);

__global__ void ffgp_copy_lower_kernel(const double* __restrict__ src, int lds_, double* __restrict__ dst, int ldd, int n) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), r = blockIdx.y * 32 + (threadIdx.x >> 5) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rr = r + k;
    if (rr < n && c <= rr) dst[(size_t)rr * ldd + c] = src[(size_t)rr * lds_ + c];
  }
}

// lower triangle -> full symmetric matrix (gradient w.r.t. a caller-built covariance)
__global__ void ffgp_symmetrize_kernel(const double* __restrict__ Gl, int ldg, double* __restrict__ out, int ldo, int n,
                                       double scale) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), r = blockIdx.y * 32 + (threadIdx.x >> 5) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rr = r + k;
    if (rr < n && c < n) out[(size_t)rr * ldo + c] = scale * ((c <= rr) ? Gl[(size_t)rr * ldg + c] : Gl[(size_t)c * ldg + rr]);
  }
}

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

static void stage_mark(ffgp_handle* h, int idx) {
  if (h->timing >= 1 && idx <= FFGP_MAX_STAGES) {
    hipEventRecord(h->ev[idx], h->stream);
    if (idx > h->n_stages) h->n_stages = idx;
  }
}

static void stage_collect(ffgp_handle* h) {
  if (h->timing < 1) return;
  for (int i = 0; i < FFGP_MAX_STAGES; ++i) h->stage_ms[i] = 0.f;
  for (int i = 0; i < h->n_stages; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]) == hipSuccess) h->stage_ms[i] = ms;
  }
}

extern "C" {

const char* ffgp_version(void) { return "ffgp 0.6 (gfx950, fp64 MFMA)"; }
int ffgp_has_dev_options(void) { return 0; }   // (always 0: kept for existing bindings)

long ffgp_graph_replays(const ffgp_handle* h) { return h ? h->graph_replays : -1; }

struct RawGraph {          // the captured forward call (option "fwd_graph", nlml_fused_enqueue)
  ffgp_problem p;
  unsigned long epoch;
  int seen;               // 1 = this signature was enqueued plainly last time (buffers are warm): capture next
  hipGraph_t graph;
  hipGraphExec_t exec;
  bool valid;
  double* stage;          // the value the graph writes
};

static void rawg_drop_one(RawGraph* r) {
  if (!r) return;
  if (r->valid) {
    hipGraphExecDestroy(r->exec);
    hipGraphDestroy(r->graph);
  }
  r->valid = false;
  r->seen = 0;
}

static void rawg_drop(ffgp_handle* h) { rawg_drop_one(h->fwdg); }

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
static int ensure_aux2(ffgp_handle* h) { return ffgp_ensure_aux2(h); }

// ROCm binds a stream to one of its hardware queues at the stream's first USE, streams on one queue run in order, and a stream that
// first appears late shares a queue with whatever is least loaded then.  The handle's third stream (head of the triangular inverse under
// the factorisation's tail) is created by the first training step of a large block -- in a process that had reserved worker streams
// before, it landed on the caller's queue and the head ran in line with the trailing updates instead of beside them (N = 4096 training
// step 3.12 -> 3.40-3.49 ms with GPU_MAX_HW_QUEUES = 6, tools/queue_probe.py).  A process that is going to put several blocks in flight
// calls this for its main handle BEFORE it creates the worker streams (fidelityfusion_amd._lib.configure_queues does).
extern "C" int ffgp_prepare_streams(ffgp_handle* h) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_CHECK(ensure_aux2(h));
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
  h->polite_m = 6144;
  h->split_rem_max = 180;
  h->super_block = 1024;
  h->splitk_min_k = 1024;
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
  h->polite64_active = 0;
  h->trsm128_max_m = 8192;
  h->trtri_overlap = 1;
  h->trtri_fill = 0;
  h->fwd_graph = 0;
  h->graph_replays = 0;
  h->fwdg = nullptr;
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
  for (int z = 0; z < FFGP_GRAD_LANES; ++z) {
    if (h->lane_ev[z]) hipEventDestroy(h->lane_ev[z]);
    if (z > 0 && h->lane_skw[z]) hipFree(h->lane_skw[z]);
  }
  if (h->lane_scal) hipFree(h->lane_scal);
  if (h->small_kbuf) hipFree(h->small_kbuf);
  if (h->train_tab) hipFree(h->train_tab);
  if (h->train_host) hipHostFree(h->train_host);
  ffgp_assemble_collect_free(h);
  if (h->bt_info_host) hipHostFree(h->bt_info_host);
  if (h->d_scal) hipFree(h->d_scal);
  if (h->d_asm) hipFree(h->d_asm);
  rawg_drop(h);
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

int ffgp_set_option(ffgp_handle* h, const char* key, double value) {
  if (!h || !key) return FFGP_ERR_ARG;
  rawg_drop(h);      // a captured call baked the old options in
  // (the switches of experiments that were measured and lost, docs/experiments.md, are gone: their keys are refused like any unknown key)
  if (!strcmp(key, "timing")) {
    h->timing = (int)value;
  } else if (!strcmp(key, "nb_outer")) {
    const int v = (int)value;
    if (v < FFGP_NB || v % FFGP_NB) return FFGP_ERR_ARG;
    h->nb_outer = v;
  } else if (!strcmp(key, "naive")) {
    h->use_naive = (int)value;
  } else if (!strcmp(key, "aux_prio")) {
    h->aux_prio = (int)value;
  } else if (!strcmp(key, "gemm_tile")) {
    const int v = (int)value;
    if (v != 0 && v != 32 && v != 64 && v != 128) return FFGP_ERR_ARG;
    h->force_ts = v;
  } else if (!strcmp(key, "batch_grad_ob")) {
    h->batch_grad_ob = value != 0.0 ? 1 : 0;
  } else if (!strcmp(key, "small_tile_threshold")) {
    h->small_tile_threshold = (int)value;
  } else if (!strcmp(key, "tile32_threshold")) {
    h->tile32_threshold = (int)value;
  } else if (!strcmp(key, "fwd_graph")) {
    h->fwd_graph = value != 0.0;
  } else if (!strcmp(key, "ho_values")) {
    if (value != 0.0 && h->ho_selftest_failed) return FFGP_ERR_ARG;      // (this process runs its kernels one at a time: see ffgp_handoff_selftest)
    h->ho_values = value != 0.0;
  } else if (!strcmp(key, "ho_gate")) {
    h->ho_gate = value != 0.0;
  } else if (!strcmp(key, "ho_timeout_ms")) {
    if (value < 1.0 || value > 600000.0) return FFGP_ERR_ARG;
    h->ho_timeout_ms = (int)value;
  } else if (!strcmp(key, "ho_withhold")) {
    h->ho_withhold = (int)value;
  } else if (!strcmp(key, "diag_excl_rows")) {
    h->diag_excl_rows = (int)value;
  } else if (!strcmp(key, "ho_defer")) {
    if (value < 0 || value > 2) return FFGP_ERR_ARG;
    h->ho_defer = (int)value;
  } else if (!strcmp(key, "polite32_pad_kb")) {
    if (value < 0 || value > 64) return FFGP_ERR_ARG;
    h->polite32_pad_kb = (int)value;
  } else if (!strcmp(key, "polite64_pad_kb")) {
    if (value < 0 || value > 64) return FFGP_ERR_ARG;
    h->polite64_pad_kb = (int)value;
  } else if (!strcmp(key, "trsm128")) {
    h->trsm128 = value != 0.0;
  } else if (!strcmp(key, "trsm128_max_m")) {
    h->trsm128_max_m = (int)value;
  } else if (!strcmp(key, "la_min_n")) {
    h->la_min_n = (int)value;
  } else if (!strcmp(key, "chase_xl")) {
    h->chase_xl = (int)value;
  } else if (!strcmp(key, "chase_xl_max_n")) {
    h->chase_xl_max_n = (int)value;
  } else if (!strcmp(key, "grad_lanes")) {
    if (value < 1.0 || value > 3.0) return FFGP_ERR_ARG;
    h->grad_lanes = (int)value;
  } else if (!strcmp(key, "train_persist")) {
    h->train_persist_off = (value == 0.0) ? 1 : 0;
  } else if (!strcmp(key, "chase_xcc")) {
    if (value < 0 || value > 15) return FFGP_ERR_ARG;
    h->chase_xcc = (int)value;
  } else if (!strcmp(key, "la_carry")) {
    h->la_carry = (int)value;
  } else if (!strcmp(key, "la_carry_n")) {
    if (value < 0) return FFGP_ERR_ARG;
    h->la_carry_n = (int)value;
  } else if (!strcmp(key, "la_carry_rows")) {
    if (value < 0) return FFGP_ERR_ARG;
    h->la_carry_rows = (int)value;
  } else if (!strcmp(key, "lookahead")) {
    h->lookahead = (int)value;
  } else if (!strcmp(key, "polite_m")) {
    h->polite_m = (int)value;
  } else if (!strcmp(key, "split_rem_max")) {
    h->split_rem_max = (int)value;
  } else if (!strcmp(key, "super_block")) {
    const int v = (int)value;
    if (v != 0 && (v < 2 * FFGP_NB || (v & (v - 1)))) return FFGP_ERR_ARG;   // 0, or a power of two >= 256
    h->super_block = v;
    h->sinv_L = nullptr;
  } else if (!strcmp(key, "asm_mm")) {
    h->asm_mm = (int)value;
  } else if (!strcmp(key, "asm_mm_grid")) {
    if (value < 1) return FFGP_ERR_ARG;
    h->asm_mm_grid = (int)value;
  } else if (!strcmp(key, "asm_mm_min")) {
    h->asm_mm_min = (int)value;
  } else if (!strcmp(key, "trtri_fill")) {
    h->trtri_fill = (int)value;
  } else if (!strcmp(key, "trtri_overlap")) {
    h->trtri_overlap = (int)value;
  } else if (!strcmp(key, "small_max_n")) {
    h->small_max_n = (int)value;
  } else if (!strcmp(key, "sb_lower")) {
    h->sb_lower = value != 0.0;
  } else if (!strcmp(key, "sb_lower_min_n")) {
    if (value < 0) return FFGP_ERR_ARG;
    h->sb_lower_min_n = (int)value;
  } else if (!strcmp(key, "sb_sym_wg")) {
    if (value < 64 || value > 65536) return FFGP_ERR_ARG;
    h->sb_sym_wg = (int)value;
  } else if (!strcmp(key, "q2_split_min_cols")) {
    h->q2_split_min_cols = (int)value;
  } else if (!strcmp(key, "small_finish")) {
    h->small2_off = (value == 0.0) ? 1 : 0;
  } else if (!strcmp(key, "small_fused")) {
    h->small_off = (value == 0.0) ? 1 : 0;
  } else if (!strcmp(key, "chase_pack")) {
    h->chase_pack = (int)value;
  } else if (!strcmp(key, "skinny_max_n")) {
    h->skinny_max_n = (int)value;
  } else if (!strcmp(key, "splitk_min_k")) {
    h->splitk_min_k = (int)value;
  } else if (!strcmp(key, "super_min_n")) {
    h->super_min_n = (int)value;
  } else {
    return FFGP_ERR_ARG;
  }
  return FFGP_OK;
}

int ffgp_assemble(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                  const double* amp, double clamp_min, const double* diag_add, const double* diag_vec, long diag_stride,
                  const double* add_mat, int ld_add, double add_all, double mean_jitter, double* K, int ldk,
                  int lower_only, int kfun, double kparam) {
  if (!h) return FFGP_ERR_ARG;
  if (kfun < FFGP_KFUN_SE || kfun > FFGP_KFUN_RQ) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_assemble_impl(h, X1, n1, X2, n2, D, w, amp, clamp_min, diag_add, diag_vec, diag_stride, add_mat, ld_add,
                            add_all, mean_jitter, K, ldk, lower_only, kfun, kparam);
}

int ffgp_potrf(ffgp_handle* h, double* A, int n, int lda) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_potrf_impl(h, A, n, n, lda, 1);
}

int ffgp_potrf_rows(ffgp_handle* h, double* A, int n, int mtot, int lda) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_potrf_impl(h, A, n, mtot, lda, 1);
}

int ffgp_trsm_lower(ffgp_handle* h, const double* L, int n, int ldl, double* B, int nrhs, int ldb) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_trsm_lower_impl(h, L, n, ldl, B, nrhs, ldb);
}

int ffgp_trsm_lower_t(ffgp_handle* h, const double* L, int n, int ldl, double* B, int nrhs, int ldb) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_trsm_lower_t_impl(h, L, n, ldl, B, nrhs, ldb);
}

int ffgp_potrs(ffgp_handle* h, const double* L, int n, int ldl, double* B, int nrhs, int ldb) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_CHECK(ffgp_trsm_lower_impl(h, L, n, ldl, B, nrhs, ldb));
  return ffgp_trsm_lower_t_impl(h, L, n, ldl, B, nrhs, ldb);
}

int ffgp_nll_reduce(ffgp_handle* h, int variant, const double* L, int n, int ldl, const double* M, int d, int ldm,
                    double pi_const, double* out_dev) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_nll_reduce_impl(h, variant, L, n, ldl, M, n, d, ldm, d, pi_const, out_dev);
}

int ffgp_gemm(ffgp_handle* h, int opa, int opb, int lower_tiles, int tri, const double* A, int lda, const double* B, int ldb,
              double* C, int ldc, int m, int n, int k, double alpha, double beta) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_gemm_launch(h, opa ? OP_MNMAJOR : OP_KMAJOR, opb ? OP_MNMAJOR : OP_KMAJOR, lower_tiles ? TILES_LOWER : TILES_FULL,
                          0, A, lda, B, ldb, C, ldc, m, n, k, alpha, beta, tri);
}

int ffgp_kernel_input_weights(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                              const double* amp, double clamp_min, int kfun, double kparam, const double* dK, int ldk,
                              double* Wt, int ldw) {
  if (!h) return FFGP_ERR_ARG;
  if (kfun < FFGP_KFUN_SE || kfun > FFGP_KFUN_RQ) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_kernel_wt_impl(h, X1, n1, X2, n2, D, w, amp, clamp_min, kfun, kparam, dK, ldk, Wt, ldw);
}

int ffgp_syevj_small(ffgp_handle* h, const double* M, int n, int ldm, int batch, long strideM, double* Q, int ldq, long strideQ,
                     double* evals, long strideE, int descending) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_syevj_small_impl(h, M, n, ldm, batch, strideM, Q, ldq, strideQ, evals, strideE, descending);
}

int ffgp_gemm_batched(ffgp_handle* h, int opa, int opb, int lower_tiles, const double* A, int lda, long strideA, const double* B,
                      int ldb, long strideB, double* C, int ldc, long strideC, int m, int n, int k, double alpha, double beta,
                      int batch) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_gemm_launch(h, opa ? OP_MNMAJOR : OP_KMAJOR, opb ? OP_MNMAJOR : OP_KMAJOR, lower_tiles ? TILES_LOWER : TILES_FULL,
                          0, A, lda, B, ldb, C, ldc, m, n, k, alpha, beta, 0, ALIAS_NONE, batch, strideA, strideB, strideC);
}

int ffgp_rows_in(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, unsigned char* found) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_rows_in_impl(h, X1, n1, X2, n2, D, found);
}

int ffgp_kernel_grad(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const double* w,
                     const double* amp, double clamp_min, int kfun, double kparam, const double* dK, int ldk, double* g_w,
                     double* g_amp, double* g_kparam) {
  if (!h) return FFGP_ERR_ARG;
  if (kfun < FFGP_KFUN_SE || kfun > FFGP_KFUN_RQ) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_kernel_grad_impl(h, X1, n1, X2, n2, D, w, amp, clamp_min, kfun, kparam, dK, ldk, g_w, g_amp, g_kparam);
}

int ffgp_assemble_pair(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_kdesc* k, int op,
                       const double* diag_add, const double* diag_vec, long diag_stride, const double* add_mat, int ld_add,
                       double add_all, double mean_jitter, double* K, int ldk, int lower_only) {
  if (!h || !k) return FFGP_ERR_ARG;
  const ffgp_ktree t = {2, FFGP_TREE_CHAIN, {op, 0, 0}, k};
  return ffgp_assemble_tree(h, X1, n1, X2, n2, D, &t, diag_add, diag_vec, diag_stride, add_mat, ld_add, add_all, mean_jitter, K, ldk,
                            lower_only);
}

int ffgp_assemble_tree(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                       const double* diag_add, const double* diag_vec, long diag_stride, const double* add_mat, int ld_add,
                       double add_all, double mean_jitter, double* K, int ldk, int lower_only) {
  if (!h || !t) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_assemble_pair_impl(h, X1, n1, X2, n2, D, t, diag_add, diag_vec, diag_stride, add_mat, ld_add, add_all,
                                 mean_jitter, K, ldk, lower_only);
}

int ffgp_kernel_grad_pair(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_kdesc* k, int op,
                          const double* dK, int ldk, const ffgp_kdesc_grads* g) {
  if (!h || !k || !g) return FFGP_ERR_ARG;
  const ffgp_ktree t = {2, FFGP_TREE_CHAIN, {op, 0, 0}, k};
  return ffgp_kernel_grad_tree(h, X1, n1, X2, n2, D, &t, dK, ldk, g);
}

int ffgp_kernel_grad_tree(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                          const double* dK, int ldk, const ffgp_kdesc_grads* g) {
  if (!h || !t || !g || t->n_leaves < 2 || t->n_leaves > 4) return FFGP_ERR_ARG;
  if (n1 <= 0 || n2 <= 0) return FFGP_OK;
  if (D <= 0 || ldk < n2) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_CHECK(ffgp_ensure_ws(h, (ffgp_grad_pair_partial_doubles(n1, n2, D, 1, t->n_leaves) + 16) * sizeof(double)));
  return ffgp_grad_pair_impl(h, X1, n1, X2, n2, D, t, dK, ldk, 1, nullptr, 0.0, h->ws, g);
}

int ffgp_kernel_input_weights_tree(ffgp_handle* h, const double* X1, int n1, const double* X2, int n2, int D, const ffgp_ktree* t,
                                   const double* dK, int ldk, double* Wt, int ldw, long leaf_stride) {
  if (!h || !t) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_pair_wt_impl(h, X1, n1, X2, n2, D, t, dK, ldk, Wt, ldw, leaf_stride);
}

/* (re)build the inverted 128x128 diagonal blocks of a factor (also the diag-kernel timing hook of tools/) */
int ffgp_trtri_diag(ffgp_handle* h, const double* L, int n, int ldl) {
  if (!h || !L) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  return ffgp_refresh_dinv(h, L, n, ldl);
}

// ---- RCCL, resolved at run time ------------------------------------------------------------------------------
#include <dlfcn.h>
typedef int (*ffgp_nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
static ffgp_nccl_allreduce_fn ffgp_resolve_allreduce() {
  // resolved exactly once, whichever host thread (one per handle / GPU) gets here first: a function-local static's
  // initialiser runs under the language's own lock
  static const ffgp_nccl_allreduce_fn fn = [] {
    ffgp_nccl_allreduce_fn f = nullptr;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);   // the copy already in the process, if any (same SONAME)
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (lib) f = reinterpret_cast<ffgp_nccl_allreduce_fn>(dlsym(lib, "ncclAllReduce"));
    if (!f) fprintf(stderr, "[ffgp] ffgp_allreduce_sum: cannot resolve ncclAllReduce from librccl.so.1 (%s)\n", dlerror());
    return f;
  }();
  return fn;
}

int ffgp_allreduce_sum(ffgp_handle* h, void* comm, double* buf_dev, int count) {
  if (!h || !comm || !buf_dev || count <= 0) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  ffgp_nccl_allreduce_fn fn = ffgp_resolve_allreduce();
  if (!fn) return FFGP_ERR_HIP;
  const int nccl_double = 8, nccl_sum = 0;   // ncclFloat64, ncclSum (rccl.h)
  const int rc = fn(buf_dev, buf_dev, (size_t)count, nccl_double, nccl_sum, comm, h->stream);
  if (rc != 0) {
    fprintf(stderr, "[ffgp] ncclAllReduce failed with %d\n", rc);
    return FFGP_ERR_HIP;
  }
  return FFGP_OK;
}

int ffgp_invalidate(ffgp_handle* h) {
  if (!h) return FFGP_ERR_ARG;
  h->dinv_L = nullptr;   // both stores are keyed on the factor's address: forget it, the next solve rebuilds them
  h->dinv_n = 0;
  h->sinv_L = nullptr;
  h->sinv_n = 0;
  return FFGP_OK;
}

int ffgp_potri(ffgp_handle* h, double* L, int n, int ldl) {
  if (!h || !L || n <= 0) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  const size_t ld = ffgp_round_up(n, 16);
  const size_t n1 = ffgp_round_up((n + 1) / 2, FFGP_NB);
  const size_t xd = (size_t)n * ld, td = n1 * n1 + 16;
  FFGP_CHECK(ffgp_ensure_ws(h, (xd + td) * sizeof(double)));
  double* X = h->ws;
  double* T = h->ws + xd;
  FFGP_CHECK(ffgp_trtri_impl(h, L, n, ldl, X, (int)ld, T));
  FFGP_CHECK(ffgp_lauum_impl(h, X, n, (int)ld, L, ldl));
  h->dinv_L = nullptr;  // the buffer no longer holds the factor
  h->sinv_L = nullptr;
  return FFGP_OK;
}

// ------------------------------------------------------------------------------------------------------------
// fused NLML (+ gradients)
// ------------------------------------------------------------------------------------------------------------
// ---- raw parameters: elementwise links around the fused call ----------------------------------------------------------------
__device__ __forceinline__ double ffgp_link_val(int kind, double p, double c) {
  switch (kind) {
    case FFGP_LINK_INV_ABS_EPS: return 1.0 / (fabs(p) + c);
    case FFGP_LINK_EXP_NEG: return exp(-p) + c;
    case FFGP_LINK_INV: return 1.0 / p + c;
    case FFGP_LINK_ABS: return fabs(p);
    case FFGP_LINK_EXP_SQ: { const double e = exp(p); return e * e; }
    case FFGP_LINK_SQUARE: return p * p + c;
    default: return p;
  }
}
__device__ __forceinline__ double ffgp_link_der(int kind, double p, double c) {
  switch (kind) {
    case FFGP_LINK_INV_ABS_EPS: { const double a = fabs(p) + c; return ((p > 0.0) ? -1.0 : ((p < 0.0) ? 1.0 : 0.0)) / (a * a); }
    case FFGP_LINK_EXP_NEG: return -exp(-p);
    case FFGP_LINK_INV: return -1.0 / (p * p);
    case FFGP_LINK_ABS: return (p > 0.0) ? 1.0 : ((p < 0.0) ? -1.0 : 0.0);
    case FFGP_LINK_EXP_SQ: { const double e = exp(p); return 2.0 * e * e; }
    case FFGP_LINK_SQUARE: return 2.0 * p;
    default: return 1.0;
  }
}
// eff = [w (D) | amp | dadd]
__global__ void ffgp_link_fwd(ffgp_links l, int D, const double* __restrict__ rw, const double* __restrict__ ramp,
                              const double* __restrict__ rdadd, double* __restrict__ eff) {
  const int t = threadIdx.x;
  if (t < D) eff[t] = ffgp_link_val(l.w_link, rw[l.w_broadcast ? 0 : t], l.w_c);
  if (t == 0) {
    eff[D] = ffgp_link_val(l.amp_link, ramp[0], l.amp_c);
    if (rdadd) eff[D + 1] = ffgp_link_val(l.dadd_link, rdadd[0], l.dadd_c);
  }
}
// the same for up to FFGP_MULTI_MAX models per launch (the members of a shared-chain batch)
struct ffgp_multi_link {
  ffgp_links l[FFGP_MULTI_MAX];
  const double* rw[FFGP_MULTI_MAX];
  const double* ramp[FFGP_MULTI_MAX];
  const double* rdadd[FFGP_MULTI_MAX];
  double* eff[FFGP_MULTI_MAX];
  int D[FFGP_MULTI_MAX];
};
__global__ void ffgp_link_fwd_multi(ffgp_multi_link q) {
  const int z = blockIdx.x, t = threadIdx.x, D = q.D[z];
  const ffgp_links& l = q.l[z];
  double* __restrict__ eff = q.eff[z];
  if (t < D) eff[t] = ffgp_link_val(l.w_link, q.rw[z][l.w_broadcast ? 0 : t], l.w_c);
  if (t == 0) {
    eff[D] = ffgp_link_val(l.amp_link, q.ramp[z][0], l.amp_c);
    if (q.rdadd[z]) eff[D + 1] = ffgp_link_val(l.dadd_link, q.rdadd[z][0], l.dadd_c);
  }
}
// geff = [g_w (D) | g_amp | g_dadd] -> gradients with respect to the raw parameters (any output pointer may be null)
__global__ void ffgp_link_bwd(ffgp_links l, int D, const double* __restrict__ rw, const double* __restrict__ ramp,
                              const double* __restrict__ rdadd, const double* __restrict__ geff, double* __restrict__ g_rw,
                              double* __restrict__ g_ramp, double* __restrict__ g_rdadd, double sc) {
  const int t = threadIdx.x;
  if (g_rw) {
    if (!l.w_broadcast) {
      if (t < D) g_rw[t] = sc * geff[t] * ffgp_link_der(l.w_link, rw[t], l.w_c);
    } else if (t == 0) {
      double s = 0.0;
      for (int k = 0; k < D; ++k) s += geff[k];
      g_rw[0] = sc * s * ffgp_link_der(l.w_link, rw[0], l.w_c);
    }
  }
  if (t == 0) {
    if (g_ramp) g_ramp[0] = sc * geff[D] * ffgp_link_der(l.amp_link, ramp[0], l.amp_c);
    if (g_rdadd && rdadd) g_rdadd[0] = sc * geff[D + 1] * ffgp_link_der(l.dadd_link, rdadd[0], l.dadd_c);
  }
}

static int nlml_fused_enqueue(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g);

// info[1] is sticky: the first failing pivot of any fused call enqueued since the last ffgp_wait
__global__ void ffgp_sticky_info_kernel(int* info) {
  if (info[1] == 0 && info[0] != 0) info[1] = info[0];
}

int ffgp_wait(ffgp_handle* h) {
  if (!h) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  stage_collect(h);
  const int rc = h->h_info[1] ? h->h_info[1] : h->h_info[0];
  if (h->h_info[1]) {
    h->h_info[1] = 0;
    FFGP_HIP(hipMemsetAsync(h->d_info + 1, 0, sizeof(int), h->stream));
  }
  return ffgp_map_info(rc);
}

int ffgp_nlml_fused_async(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g) {
  return nlml_fused_enqueue(h, p, nll_dev, g);
}

int ffgp_nlml_fused(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g) {
  FFGP_CHECK(nlml_fused_enqueue(h, p, nll_dev, g));
  return ffgp_wait(h);
}

__global__ void ffgp_scale_outputs(double sc, double* __restrict__ nll, double* __restrict__ gY, long nY, double* __restrict__ gv, long nv,
                                   double* __restrict__ gk) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) {
    nll[0] *= sc;
    if (gk) gk[0] *= sc;
  }
  if (gY && t < nY) gY[t] *= sc;
  if (gv && t < nv) gv[t] *= sc;
}

static int nlml_fused_raw_enqueue(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g);

int ffgp_nlml_fused_raw(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  FFGP_CHECK(nlml_fused_raw_enqueue(h, p, l, nll_dev, g));
  return ffgp_wait(h);
}

int ffgp_nlml_fused_raw_async(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  return nlml_fused_raw_enqueue(h, p, l, nll_dev, g);
}

int ffgp_nlml_fused_small_batch_async(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, double* nll_dev,
                                      const ffgp_grads* g) {
  if (!h || !p || !nll_dev || F <= 0) return FFGP_ERR_ARG;
  for (int f = 0; f < F; ++f)
    if (!ffgp_small_batch_ok(p + f, g ? g + f : nullptr)) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  h->n_stages = 0;
  FFGP_CHECK(ffgp_zero_async(h, h->d_info, sizeof(int)));
  bool mfma = true;      // (round 6: the one-workgroup MFMA kernel of train.hip, when every problem is within its limits)
  for (int f = 0; f < F && mfma; ++f) mfma = ffgp_small_mfma_ok(h, p + f, g ? g + f : nullptr);
  if (mfma) FFGP_CHECK(ffgp_small_mfma_enqueue(h, F, p, l, nll_dev, g, 1));
  else FFGP_CHECK(ffgp_small_batch_enqueue(h, F, p, l, nll_dev, g));
  if (!h->fold_info) hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
  if (!h->defer_info_copy) FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return FFGP_OK;
}

int ffgp_nlml_fused_small_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  FFGP_CHECK(ffgp_nlml_fused_small_batch_async(h, F, p, l, nll_dev, g));
  return ffgp_wait(h);
}

// streams, events and scalar scratch of the gradient lanes (ffgp_nlml_fused_batch), created at first use
static int ffgp_grad_lanes_prepare(ffgp_handle* h, int nl) {
  if (!h->lane_scal) {
    FFGP_HIP(hipMalloc(&h->lane_scal, (size_t)FFGP_GRAD_LANES * 64 * sizeof(double)));
    FFGP_HIP(hipMemsetAsync(h->lane_scal, 0, (size_t)FFGP_GRAD_LANES * 64 * sizeof(double), h->stream));
  }
  // the lanes are the handle's side streams (idle during the gradient stages): they own hardware queues already -- a stream created
  // now would be dealt onto one of the few queues round robin, quite possibly the call's own, and run BEHIND it
  FFGP_CHECK(ffgp_ensure_aux2(h));
  h->lane_st[1] = h->aux2;
  h->lane_st[2] = h->aux3;      // (not the chain's stream h->aux: the GEMM launcher treats launches on it specially -- priority, no split-K)
  for (int z = 0; z < nl; ++z)
    if (!h->lane_ev[z]) FFGP_HIP(hipEventCreateWithFlags(&h->lane_ev[z], hipEventDisableTiming));
  return FFGP_OK;
}

// ---- F blocks of ONE shape in one chain of launches ----------------------------------------------------------------------------
// The reference's per-fidelity / per-seed loops evaluate independent blocks of equal size one after the other
// (Experiments/GAR_Aligned/exp_aligned.py:58-126, FidelityFusion_Models/ResGP.py:78-112).  Below N ~ 6000 a block's
// factorisation is a dependency chain of a few hundred short launches (32 diagonal blocks x (factor 32 us + solve 11 + update 8) at
// N = 4096: 1.9 of the 2.0 ms); overlapping blocks through streams gives each block its own chain on a shared chip (eight C2 blocks:
// 1.5 ms each).  Here the F blocks sit at a fixed stride in one workspace and every launch of the chain covers all of them -- the
// diagonal-block kernel runs one workgroup per block, the GEMMs carry the block index in gridDim.y -- so F blocks share ONE chain
// and fill its gaps with F times the matrix-core work.  The per-block arithmetic is the single call's, instruction for instruction
// (same kernels, same k order): the values are bit-identical to F separate calls.
// Conditions (else FFGP_ERR_ARG, and the caller falls back to separate calls): 2 <= F <= 256 blocks with n > 128, V1
// likelihood, one radial-profile kernel each (no pair / tree / caller-built covariance), not the naive kernels.
// Round 5: the blocks may have DIFFERENT n and d (the reference's fidelities are ragged by nature, FidelityFusion_Models/ResGP.py:121-136):
// every member follows its own single call's launch sequence and launches of the same kind at the same chain step are merged
// (ffgp_potrf_ragged, ffgp_gemm_launch_rag), members drop out as their columns run out; members above 12288 rows are refused.
// Gradients: the factorisation is shared, the inverse / gradient stages run block after block on the shared scratch.
int ffgp_nlml_fused_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g,
                          int* status) {
  if (!h || !p || !nll_dev || F < 2 || F > 256) return FFGP_ERR_ARG;
  if (h->use_naive) return FFGP_ERR_ARG;
  bool want_grad = false, uniform = true;
  for (int f = 0; f < F; ++f) {
    const ffgp_problem& q = p[f];
    if (q.n <= FFGP_NB || q.d <= 0 || q.cov_dev || q.pair || q.tree || !q.X_dev || !q.Y_dev || !q.w_dev || !q.amp_dev || q.D <= 0 || q.D > 128 ||
        q.ll_variant != FFGP_LL_V1 || q.kfun < FFGP_KFUN_SE || q.kfun > FFGP_KFUN_RQ)
      return FFGP_ERR_ARG;
    uniform = uniform && q.n == p[0].n && q.d == p[0].d;
    if (g) {
      const ffgp_grads& gg = g[f];
      if (gg.g_cov_dev || gg.g_pair) return FFGP_ERR_ARG;
      want_grad = want_grad || gg.g_w_dev || gg.g_amp_dev || gg.g_diag_add_dev || gg.g_Y_dev || gg.g_diag_vec_dev || gg.g_kparam_dev;
    }
  }
  if (!uniform) {      // members of different sizes: the ragged chain's own limits (ffgp_potrf_ragged)
    for (int f = 0; f < F; ++f)
      if (h->lookahead && p[f].n > h->nb_outer && p[f].n > h->la_min_n && !(h->la_carry == 1 || (h->la_carry == 2 && p[f].n <= h->la_carry_n)))
        return FFGP_ERR_ARG;
  }
  FFGP_HIP(hipSetDevice(h->device));
  // per-member layout: [Sigma | Y^T] -> [L | Gamma^T] blocks one after the other, each with its own leading dimension
  std::vector<size_t> ldv(F), offv(F), doffv(F);
  std::vector<int> nblkv(F);
  size_t total = 0, dinv_blocks = 0, sX = 0, sT = 0, sAt = 0, sP = 0;
  int Dmax = 0;
  for (int f = 0; f < F; ++f) {
    const int n = p[f].n, d = p[f].d;
    ldv[f] = ffgp_round_up(n, 16);
    offv[f] = total;
    total += (size_t)(n + d) * ldv[f];
    nblkv[f] = (n + FFGP_NB - 1) / FFGP_NB;
    doffv[f] = dinv_blocks * FFGP_NB * FFGP_NB;
    dinv_blocks += nblkv[f];
    const size_t n1 = ffgp_round_up((n + 1) / 2, FFGP_NB);
    sX = std::max(sX, (size_t)n * ldv[f]);
    sT = std::max(sT, 2 * (n1 * n1 + 16));
    sAt = std::max(sAt, (size_t)d * ldv[f]);
    sP = std::max(sP, (size_t)ffgp_grad_partial_doubles(n, p[f].D) + 16);
    Dmax = p[f].D > Dmax ? p[f].D : Dmax;
  }
  const size_t blk = offv.size() > 1 ? offv[1] - offv[0] : total;     // (uniform batches: the stride between the blocks)
  const size_t o_link = total; total += (size_t)F * 512;   // effective parameters / their gradients, 256 + 256 doubles per block
  const size_t o_red = total; total += (size_t)F * 2 * FFGP_RED_BLOCKS;   // partial sums of the members' reductions
  size_t o_X = 0, o_S = 0, o_T = 0, o_At = 0, o_P = 0;
  // gradient stage: when EVERY block of an equal-shape batch wants gradients (and the inverses fit), Sigma_f^-1 of all blocks come out
  // of one sequence of launches with an outer batch index (ffgp_trtri_lauum_ob) -- a lone N = 4096 inverse underfills the chip at its
  // lower levels; otherwise block after block through one set of buffers
  bool all_grad = want_grad && g && h->batch_grad_ob && uniform;
  for (int f = 0; f < F && all_grad; ++f) {
    const ffgp_grads& gg = g[f];
    all_grad = gg.g_w_dev || gg.g_amp_dev || gg.g_diag_add_dev || gg.g_Y_dev || gg.g_diag_vec_dev || gg.g_kparam_dev;
  }
  if (all_grad && (size_t)F * (2 * sX + sT) * sizeof(double) > ((size_t)48 << 30)) all_grad = false;
  // Members whose gradient stages cannot share launches (different sizes) run them SIDE BY SIDE instead (round 6): up to four lanes, each
  // a stream with its own scratch (inverse, Sigma^-1, TRTRI workspace, A^T, partial sums, split-K workspace, trace scalar), every member's
  // stage sequence exactly its single call's -- so its bits are too.  For three blocks of 300 / 300 / 250 points the three latency-bound
  // chains of ~12 launches overlap; larger members fill one another's gaps.  Option "grad_lanes" (default 4; 1 = member after member).
  int n_grad = 0;
  if (want_grad && g)
    for (int f = 0; f < F; ++f) {
      const ffgp_grads& gg = g[f];
      n_grad += (gg.g_w_dev || gg.g_amp_dev || gg.g_diag_add_dev || gg.g_Y_dev || gg.g_diag_vec_dev || gg.g_kparam_dev) ? 1 : 0;
    }
  int nmax_all = 0;
  for (int f = 0; f < F; ++f) nmax_all = std::max(nmax_all, p[f].n);
  // measured (tools/ragged_probe.py, FFGP_OPTS=grad_lanes=1 / 3): (300, 300, 250) 0.839 -> 0.789 ms, (4096, 3000, 2000) 5.32 -> 5.02,
  // (2048, 2048, 1024, 1500) 2.77 -> 2.69; (8192, 4096, 2048, 1024) 16.3 -> 17.0 -- a throughput-bound member gains nothing from
  // neighbours on its chip, so sets with a member above 6144 rows stay member after member.  Small members are bound by the HOST's
  // launch rate (15 launches per member), which lanes do not change: the gate of 1.4 x the largest member is not met (1.66 x).
  int nl = (!all_grad && n_grad >= 2 && h->grad_lanes > 1 && h->timing == 0 && nmax_all <= 6144) ? std::min(std::min(n_grad, h->grad_lanes), 3) : 1;
  sT = (sT + 15) / 16 * 16; sAt = (sAt + 15) / 16 * 16; sP = (sP + 15) / 16 * 16;
  if (nl > 1 && (size_t)nl * (2 * sX + sT) * sizeof(double) > ((size_t)48 << 30)) nl = 1;
  const size_t copies = all_grad ? (size_t)F : (size_t)nl;
  if (want_grad) {
    o_X = total; total += copies * sX;
    o_S = total; total += copies * sX;
    o_T = total; total += copies * sT;
    o_At = total; total += (size_t)nl * sAt;
    o_P = total; total += (size_t)nl * sP;
  }
  FFGP_CHECK(ffgp_ensure_ws(h, total * sizeof(double)));
  if (!h->bt_info) {
    FFGP_HIP(hipMalloc(&h->bt_info, 256 * sizeof(int)));
    FFGP_HIP(hipHostMalloc(&h->bt_info_host, 256 * sizeof(int)));
  }
  FFGP_CHECK(ffgp_ensure_dinv(h, (int)(dinv_blocks * FFGP_NB)));
  FFGP_CHECK(ffgp_zero_async(h, h->bt_info, (size_t)F * sizeof(int)));
  h->n_stages = 0;
  stage_mark(h, 0);
  // ---- links, assembly, passenger rows: block after block (each a few launches that fill the chip by themselves)
  // (the tiny per-member stages -- links, target transposes, the reductions further down -- are issued for eight members per launch:
  // F x 5 launches of a few microseconds each were a third of a 300 / 300 / 250 batch's time)
  ffgp_problem* q = (ffgp_problem*)alloca(sizeof(ffgp_problem) * F);
  for (int f = 0; f < F; ++f) {
    q[f] = p[f];
    double* eff = h->ws + o_link + (size_t)f * 512;
    if (l) {
      q[f].w_dev = eff;
      q[f].amp_dev = eff + p[f].D;
      if (p[f].diag_add_dev) q[f].diag_add_dev = eff + p[f].D + 1;
    }
  }
  if (l) {
    for (int f0 = 0; f0 < F; f0 += FFGP_MULTI_MAX) {
      const int cnt = F - f0 < FFGP_MULTI_MAX ? F - f0 : FFGP_MULTI_MAX;
      ffgp_multi_link ml;
      for (int z = 0; z < FFGP_MULTI_MAX; ++z) {
        const int f = f0 + (z < cnt ? z : 0);
        ml.l[z] = l[f]; ml.rw[z] = p[f].w_dev; ml.ramp[z] = p[f].amp_dev; ml.rdadd[z] = p[f].diag_add_dev;
        ml.eff[z] = h->ws + o_link + (size_t)f * 512; ml.D[z] = p[f].D;
      }
      hipLaunchKernelGGL(ffgp_link_fwd_multi, dim3(cnt), dim3(128), 0, h->stream, ml);
    }
  }
  {
    std::vector<const double*> tsrc(F);
    std::vector<double*> tdst(F);
    std::vector<int> trows(F), tcols(F), tlds(F), tldd(F);
    ffgp_assemble_collect_begin(h);      // (small members' assemblies: parked, then eight per launch)
    int arc = FFGP_OK;
    for (int f = 0; f < F && arc == FFGP_OK; ++f) {
      const int n = p[f].n, d = p[f].d;
      double* W0 = h->ws + offv[f];
      arc = ffgp_assemble_impl(h, q[f].X_dev, n, q[f].X_dev, n, q[f].D, q[f].w_dev, q[f].amp_dev, q[f].clamp_min, q[f].diag_add_dev,
                               q[f].diag_vec_dev, q[f].diag_stride, q[f].add_mat_dev, q[f].ld_add, q[f].add_all, q[f].mean_jitter, W0,
                               (int)ldv[f], 1, q[f].kfun, q[f].kparam);
      tsrc[f] = q[f].Y_dev; tdst[f] = W0 + (size_t)n * ldv[f]; trows[f] = n; tcols[f] = d; tlds[f] = d; tldd[f] = (int)ldv[f];
    }
    const int erc = ffgp_assemble_collect_end(h);      // (always: the handle must not stay in collecting mode)
    FFGP_CHECK(arc);
    FFGP_CHECK(erc);
    FFGP_CHECK(ffgp_transpose_multi(h, F, tsrc.data(), trows.data(), tcols.data(), tlds.data(), tdst.data(), tldd.data()));
  }
  stage_mark(h, 1);
  // ---- ONE factorisation chain for all F blocks
  h->tri_hook_col = 0;
  h->tri_hook_fired = 0;
  int prc;
  if (uniform) {
    h->bt_F = F;
    h->bt_sA = (long)blk;
    h->bt_sD = (long)nblkv[0] * FFGP_NB * FFGP_NB;
    prc = ffgp_potrf_impl(h, h->ws, p[0].n, p[0].n + p[0].d, (int)ldv[0], 0);
    h->bt_F = 0;
  } else {
    std::vector<ffgp_rag_block> mem(F);
    for (int f = 0; f < F; ++f) mem[f] = ffgp_rag_block{h->ws + offv[f], p[f].n, p[f].n + p[f].d, (int)ldv[f], h->dinv + doffv[f], f};
    prc = ffgp_potrf_ragged(h, F, mem.data());
  }
  h->dinv_L = nullptr;          // (the store holds F factors' inverses: it belongs to none of them as far as the cache is concerned)
  h->sinv_L = nullptr;
  FFGP_CHECK(prc);
  stage_mark(h, 2);
  double* const dinv0 = h->dinv;
  int rc_stage = FFGP_OK;
  if (all_grad)
    rc_stage = ffgp_trtri_lauum_ob(h, F, h->ws, (long)blk, p[0].n, (int)ldv[0], h->ws + o_X, (long)sX, (int)ldv[0], h->ws + o_T, (long)sT,
                                   h->ws + o_S, (long)sX, (int)ldv[0], dinv0, (long)nblkv[0] * FFGP_NB * FFGP_NB);
  const bool fwd_only = !(want_grad && g);
  if (rc_stage == FFGP_OK) {
    std::vector<const double*> rL(F), rM(F);
    std::vector<double*> rout(F);
    std::vector<int> rn(F), rld(F), rd(F);
    std::vector<double> rpi(F), rsc(F);
    for (int f = 0; f < F; ++f) {
      rL[f] = h->ws + offv[f]; rM[f] = h->ws + offv[f] + (size_t)p[f].n * ldv[f]; rout[f] = nll_dev + f;
      rn[f] = p[f].n; rld[f] = (int)ldv[f]; rd[f] = p[f].d; rpi[f] = q[f].pi_const;
      // forward only: the output scale (the sign of the reference's +LL) is folded into the reduction's last step
      rsc[f] = (l && fwd_only && l[f].out_scale != 0.0) ? l[f].out_scale : 1.0;
    }
    rc_stage = ffgp_nll_reduce_multi(h, F, rL.data(), rn.data(), rld.data(), rM.data(), rd.data(), rn.data(), rld.data(), rd.data(), rpi.data(),
                                     rsc.data(), rout.data(), h->ws + o_red);
  }
  // lanes: members dealt longest-first to the lane with the least work so far; lane 0 is the call's own stream
  std::vector<int> order(F), lane_of(F, 0);
  for (int f = 0; f < F; ++f) order[f] = f;
  hipStream_t const main_stream = h->stream;
  if (nl > 1 && rc_stage == FFGP_OK) {
    rc_stage = ffgp_grad_lanes_prepare(h, nl);
    if (rc_stage == FFGP_OK) {
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p[a].n > p[b].n; });
      double load[FFGP_GRAD_LANES] = {0.0, 0.0, 0.0, 0.0};
      for (int f : order) {
        int best = 0;
        for (int z = 1; z < nl; ++z)
          if (load[z] < load[best]) best = z;
        lane_of[f] = best;
        load[best] += (double)p[f].n * p[f].n * p[f].n + 1e6;      // (+ a launch-count term: small members are chains of launches)
      }
      if (hipEventRecord(h->lane_ev[0], main_stream) != hipSuccess) rc_stage = FFGP_ERR_HIP;
      for (int z = 1; z < nl && rc_stage == FFGP_OK; ++z)
        if (hipStreamWaitEvent(h->lane_st[z], h->lane_ev[0], 0) != hipSuccess) rc_stage = FFGP_ERR_HIP;
    }
  }
  struct LaneGuard {      // the handle's stream and per-lane scratch pointers while one member's stages are enqueued on a lane
    ffgp_handle* h; int lane; hipStream_t main_s; double* skw0; size_t skwb0; double* scal0;
    LaneGuard(ffgp_handle* h_, int lane_, hipStream_t m) : h(h_), lane(lane_), main_s(m), skw0(h_->skw), skwb0(h_->skw_bytes), scal0(h_->d_scal) {
      if (lane > 0) {
        h->stream = h->lane_st[lane];
        h->skw = h->lane_skw[lane]; h->skw_bytes = h->lane_skw_bytes[lane];
        h->d_scal = h->lane_scal + (size_t)lane * 64;
      }
    }
    ~LaneGuard() {
      if (lane > 0) {
        h->lane_skw[lane] = h->skw; h->lane_skw_bytes[lane] = h->skw_bytes;      // (it may have grown)
        h->skw = skw0; h->skw_bytes = skwb0; h->d_scal = scal0;
        h->stream = main_s;
      }
    }
  };
  for (int oi = 0; oi < F && rc_stage == FFGP_OK; ++oi) {
    const int f = order[oi];
    const int n = p[f].n, d = p[f].d;
    const int ld = (int)ldv[f];
    double* W0 = h->ws + offv[f];
    double* Gt = W0 + (size_t)n * ld;
    if (!want_grad || !g) continue;
    const ffgp_grads& gg = g[f];
    if (!(gg.g_w_dev || gg.g_amp_dev || gg.g_diag_add_dev || gg.g_Y_dev || gg.g_diag_vec_dev || gg.g_kparam_dev)) continue;
    const int lane = (nl > 1) ? lane_of[f] : 0;
    LaneGuard lg(h, lane, main_stream);
    // the block's own slice of the Dinv store, presented as "the" store of this factor while its inverse is formed
    h->dinv = dinv0 + doffv[f];
    h->dinv_L = W0; h->dinv_n = n; h->dinv_ld = ld;
    double* X = h->ws + o_X + (all_grad ? (size_t)f * sX : (size_t)lane * sX);
    double* S = h->ws + o_S + (all_grad ? (size_t)f * sX : (size_t)lane * sX);
    double* T = h->ws + o_T + (all_grad ? 0 : (size_t)lane * sT);
    double* At = h->ws + o_At + (size_t)lane * sAt;
    double* P = h->ws + o_P + (size_t)lane * sP;
    double* geff = h->ws + o_link + (size_t)f * 512 + 256;
    const int D = q[f].D;
    ffgp_grads gq = gg;
    bool chain = false;
    if (l) {
      if (gg.g_w_dev) gq.g_w_dev = geff;
      if (gg.g_amp_dev) gq.g_amp_dev = geff + D;
      if (gg.g_diag_add_dev) gq.g_diag_add_dev = geff + D + 1;
      chain = gg.g_w_dev || gg.g_amp_dev || gg.g_diag_add_dev;
    }
    if (!all_grad) {
      if ((rc_stage = ffgp_trtri_impl(h, W0, n, ld, X, ld, T)) != FFGP_OK) break;
      if ((rc_stage = ffgp_lauum_impl(h, X, n, ld, S, ld)) != FFGP_OK) break;
    }
    if ((rc_stage = ffgp_gemm_launch(h, OP_KMAJOR, OP_MNMAJOR, TILES_FULL, 0, Gt, ld, X, ld, At, ld, d, n, n, 1.0, 0.0,
                                     TRI_LO_J)) != FFGP_OK) break;
    if ((rc_stage = ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_LOWER, 0, At, ld, At, ld, S, ld, n, n, d, -0.5,
                                     0.5 * (double)d)) != FFGP_OK) break;
    if ((rc_stage = ffgp_grad_impl(h, q[f].X_dev, n, D, q[f].w_dev, q[f].amp_dev, q[f].clamp_min, S, ld, q[f].mean_jitter, gq.g_w_dev,
                                   gq.g_amp_dev, gq.g_diag_add_dev, gq.g_diag_vec_dev, P, q[f].kfun, q[f].kparam, gq.g_kparam_dev)) != FFGP_OK) break;
    if (gg.g_Y_dev && (rc_stage = ffgp_transpose(h, At, d, n, ld, gg.g_Y_dev, d, 1.0)) != FFGP_OK) break;
    if (l) {
      const double sc = (l[f].out_scale == 0.0) ? 1.0 : l[f].out_scale;
      if (chain)
        hipLaunchKernelGGL(ffgp_link_bwd, dim3(1), dim3(128), 0, h->stream, l[f], D, p[f].w_dev, p[f].amp_dev, p[f].diag_add_dev, geff,
                           gg.g_w_dev, gg.g_amp_dev, gg.g_diag_add_dev, sc);
      if (sc != 1.0) {
        const long nY = gg.g_Y_dev ? (long)n * d : 0, nv = gg.g_diag_vec_dev ? n : 0;
        const long tot = nY > nv ? nY : nv;
        hipLaunchKernelGGL(ffgp_scale_outputs, dim3((unsigned)((tot > 0 ? tot : 1) + 255) / 256), dim3(256), 0, h->stream, sc, nll_dev + f,
                           gg.g_Y_dev, nY, gg.g_diag_vec_dev, nv, gg.g_kparam_dev);
      }
    }
  }
  h->dinv = dinv0;
  h->dinv_L = nullptr;
  if (nl > 1) {      // the call's stream waits for every lane (also on an error path: nothing of this call may still be running on a lane)
    for (int z = 1; z < nl; ++z) {
      if (hipEventRecord(h->lane_ev[z], h->lane_st[z]) != hipSuccess || hipStreamWaitEvent(main_stream, h->lane_ev[z], 0) != hipSuccess) {
        (void)hipGetLastError();
        hipStreamSynchronize(h->lane_st[z]);
      }
    }
  }
  FFGP_CHECK(rc_stage);
  if (l && fwd_only) {      // forward only: the output scale was applied by the reduction
  } else if (l) {                   // blocks without gradients of their own inside a gradient batch
    for (int f = 0; f < F; ++f) {
      const ffgp_grads& gg = g[f];
      const double sc = (l[f].out_scale == 0.0) ? 1.0 : l[f].out_scale;
      if (!(gg.g_w_dev || gg.g_amp_dev || gg.g_diag_add_dev || gg.g_Y_dev || gg.g_diag_vec_dev || gg.g_kparam_dev) && sc != 1.0)
        hipLaunchKernelGGL(ffgp_scale_outputs, dim3(1), dim3(256), 0, h->stream, sc, nll_dev + f, (double*)nullptr, 0L, (double*)nullptr, 0L,
                           (double*)nullptr);
    }
  }
  stage_mark(h, 3);
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  FFGP_HIP(hipMemcpyAsync(h->bt_info_host, h->bt_info, (size_t)F * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  if (h->timing) stage_collect(h);
  int first = FFGP_OK;
  for (int f = 0; f < F; ++f) {
    const int v = ffgp_map_info(h->bt_info_host[f]);
    if (status) status[f] = v;
    if (v != 0 && first == FFGP_OK) first = v;
  }
  return first;
}

// ---- K training steps in ONE call -------------------------------------------------------------------------------------------
// The reference's hot loop (FidelityFusion_Models/ResGP.py:78-112: per fidelity 100-1000 iterations of zero_grad / loss =
// -negative_log_likelihood / backward / Adam step at N = 16 ... 500) costs one Python round trip, one autograd graph and one status
// read-back per iteration through the drop-in modules -- 0.28-0.32 ms at N <= 128, of which 0.125 ms is GPU work.  Here the whole
// loop is enqueued by one call: per step the likelihood + closed-form gradients on the raw parameters (the same launches as
// ffgp_nlml_fused_raw, or ONE launch for all models when they are small: ffgp_nlml_fused_small_batch's kernel) and one Adam
// kernel that updates the raw parameters IN PLACE on the device (torch.optim.Adam's arithmetic, operation for operation: lerp,
// mul + addcmul, bias corrections computed on the host with the C library's pow as Python does, sqrt / div / add eps, addcdiv) and
// stores the step's loss in the trace.  No host synchronisation inside the loop; the factorisation status is sticky and read once
// at the end (the first step whose Sigma was not positive definite; the parameters stop moving from that step on).
__global__ void ffgp_adam_kernel(int F, ffgp_train_slot sl, const double* __restrict__ gbuf, double* __restrict__ state, long state_stride,
                                 double lr, double b1, double b2, double eps, double bc1, double bc2_sqrt, const double* __restrict__ loss,
                                 double* __restrict__ trace, long trace_stride, int step, int* __restrict__ info, int fold,
                                 const double* __restrict__ geff, ffgp_links lk, int lD, double lsc) {
  const int f = blockIdx.x;
  if (f >= F) return;
  const int i0 = info[0], i1 = info[1];
  const int bad = i0 | i1;
  if (fold) {      // (one model per call: this kernel also keeps the status words -- sticky first failure, current word cleared for the
    __syncthreads();   //  next step's factorisation -- two single-thread launches per step otherwise)
    if (threadIdx.x == 0) {
      if (i1 == 0 && i0 != 0) info[1] = i0;
      info[0] = 0;
    }
  }
  const int nw = sl.nw[f];
  const int npar = nw + 2 + (sl.rho[f] ? 1 : 0);      // (a residual member's rho is the last parameter; its gradient is in gbuf)
  if (threadIdx.x == 0) trace[(size_t)f * trace_stride + step] = bad ? __builtin_nan("") : loss[f];
  if (bad) return;
  const int i = threadIdx.x;
  if (i >= npar) return;
  double* par = (i < nw) ? sl.w[f] + i : (i == nw ? sl.amp[f] : (i == nw + 1 ? sl.dadd[f] : sl.rho[f]));
  double g;
  if (i == nw + 2) {
    g = gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + i];
  } else if (geff) {
    // (one model, blocked path: the gradients arrive with respect to the EFFECTIVE parameters [w (D) | amp | diag_add]; the links'
    //  chain rule -- ffgp_link_bwd's arithmetic -- is applied here instead of in a launch of its own)
    if (i < nw) {
      if (!lk.w_broadcast) {
        g = lsc * geff[i] * ffgp_link_der(lk.w_link, par[0], lk.w_c);
      } else {
        double sg = 0.0;
        for (int k = 0; k < lD; ++k) sg += geff[k];
        g = lsc * sg * ffgp_link_der(lk.w_link, par[0], lk.w_c);
      }
    } else if (i == nw) {
      g = lsc * geff[lD] * ffgp_link_der(lk.amp_link, par[0], lk.amp_c);
    } else {
      g = lsc * geff[lD + 1] * ffgp_link_der(lk.dadd_link, par[0], lk.dadd_c);
    }
  } else {
    g = gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + i];
  }
  double* m = state + (size_t)f * state_stride + i;
  double* v = m + npar;
  const double m1 = m[0] + (g - m[0]) * (1.0 - b1);        // exp_avg.lerp_(grad, 1 - beta1)
  const double v1 = v[0] * b2 + (1.0 - b2) * g * g;        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  m[0] = m1;
  v[0] = v1;
  const double denom = sqrt(v1) / bc2_sqrt + eps;
  par[0] = par[0] + (-(lr / bc1)) * (m1 / denom);          // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// residual members of the launch-per-stage loop (ffgp_train_residual_raw): per step their targets and diagonal extra are formed from rho
// before the likelihood call, and dloss/drho is reduced from its dloss/dY and dloss/ddiag_vec after it
struct ffgp_resid_slot {
  const double* rho[FFGP_TRAIN_MAXF];
  const double* yl[FFGP_TRAIN_MAXF];
  const double* yh[FFGP_TRAIN_MAXF];
  const double* vl[FFGP_TRAIN_MAXF];
  const double* vh[FFGP_TRAIN_MAXF];
  long vls[FFGP_TRAIN_MAXF], vhs[FFGP_TRAIN_MAXF];
  double* r[FFGP_TRAIN_MAXF];            // [n, d] targets
  double* dv[FFGP_TRAIN_MAXF];           // [n] |s|
  const double* gY[FFGP_TRAIN_MAXF];     // [n, d] dloss/dr
  const double* gdv[FFGP_TRAIN_MAXF];    // [n] dloss/ddvec
  double* rho_last[FFGP_TRAIN_MAXF];
  long nd[FFGP_TRAIN_MAXF];
  int n[FFGP_TRAIN_MAXF], nw[FFGP_TRAIN_MAXF];
};
// r = y_high - rho y_low, dvec = |v_high - rho v_low| (a product, then a difference: torch's rounding); rho_last = rho
__global__ void ffgp_resid_form(ffgp_resid_slot rs) {
  const int f = blockIdx.y;
  if (!rs.rho[f]) return;
  const double rho = rs.rho[f][0];
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < rs.nd[f]) rs.r[f][t] = __dsub_rn(rs.yh[f][t], __dmul_rn(rho, rs.yl[f][t]));
  if (rs.vl[f] && t < rs.n[f]) rs.dv[f][t] = fabs(__dsub_rn(rs.vh[f][t * rs.vhs[f]], __dmul_rn(rho, rs.vl[f][t * rs.vls[f]])));
  if (t == 0 && rs.rho_last[f]) rs.rho_last[f][0] = rho;
}
// gbuf slot nw + 2 <- dloss/drho = -sum gY .* y_low - sum_i gdv_i sgn(s_i) v_low,ii (one workgroup per member, fixed order)
__global__ void ffgp_resid_grad(ffgp_resid_slot rs, double* __restrict__ gbuf) {
  const int f = blockIdx.x;
  if (!rs.rho[f]) return;
  __shared__ double part[256];
  const double rho = rs.rho[f][0];
  double x = 0.0;
  for (long t = threadIdx.x; t < rs.nd[f]; t += 256) x = __builtin_fma(rs.gY[f][t], rs.yl[f][t], x);
  if (rs.vl[f]) {
    for (int i = threadIdx.x; i < rs.n[f]; i += 256) {
      const double vl = rs.vl[f][(long)i * rs.vls[f]];
      const double s = __dsub_rn(rs.vh[f][(long)i * rs.vhs[f]], __dmul_rn(rho, vl));
      x = __builtin_fma(rs.gdv[f][i], (s > 0.0) ? vl : ((s < 0.0) ? -vl : 0.0), x);      // (sgn(0) = 0: torch's abs backward)
    }
  }
  part[threadIdx.x] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) gbuf[(size_t)f * FFGP_TRAIN_GSTRIDE + rs.nw[f] + 2] = -part[0];
}

static int train_impl(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_residual* r, int steps,
                      const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  if (!h || !p || !l || !opt || !state_dev || !trace_dev || F <= 0 || F > FFGP_TRAIN_MAXF || steps <= 0 || step0 < 0 || trace_stride < steps)
    return FFGP_ERR_ARG;
  ffgp_train_slot sl;
  bool all_small = true, any_res = false;
  for (int f = 0; f < F; ++f) {
    const ffgp_problem& q = p[f];
    if (!q.w_dev || !q.amp_dev || !q.diag_add_dev || q.cov_dev || q.pair || q.tree || q.D <= 0 || q.D > 128 || q.n <= 0 || q.d <= 0) return FFGP_ERR_ARG;
    const bool res = r && r[f].rho_dev;
    if (res && (!r[f].y_low_dev || !r[f].y_high_dev || !q.X_dev || (!r[f].v_low_dev) != (!r[f].v_high_dev) ||
                (r[f].v_low_dev && (r[f].v_low_stride < 0 || r[f].v_high_stride < 0))))
      return FFGP_ERR_ARG;
    const int nw = l[f].w_broadcast ? 1 : q.D;
    if (state_stride < 2 * (nw + 2 + (res ? 1 : 0))) return FFGP_ERR_ARG;
    sl.w[f] = const_cast<double*>(q.w_dev);
    sl.amp[f] = const_cast<double*>(q.amp_dev);
    sl.dadd[f] = const_cast<double*>(q.diag_add_dev);
    sl.rho[f] = res ? r[f].rho_dev : nullptr;
    sl.nw[f] = nw;
    any_res = any_res || res;
  }
  FFGP_HIP(hipSetDevice(h->device));
  {   // every model small enough for one workgroup: the whole loop is ONE launch (train.hip)
    bool persist = true;
    for (int f = 0; f < F && persist; ++f) persist = ffgp_train_persist_ok(h, p + f, l + f, r ? r + f : nullptr);
    if (persist) return ffgp_train_persist(h, F, p, l, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride, r);
  }
  if (!h->train_g) {
    FFGP_HIP(hipMalloc(&h->train_g, (size_t)FFGP_TRAIN_MAXF * (FFGP_TRAIN_GSTRIDE + 1) * sizeof(double)));
  }
  double* gbuf = h->train_g;
  double* loss = h->train_g + (size_t)FFGP_TRAIN_MAXF * FFGP_TRAIN_GSTRIDE;
  std::vector<ffgp_grads> g(F);
  std::vector<ffgp_links> lk(l, l + F);
  std::vector<ffgp_problem> pq(p, p + F);      // (residual members: targets and diagonal extra in the call's own buffers)
  ffgp_resid_slot rs;
  memset(&rs, 0, sizeof(rs));
  double* rbuf = nullptr;
  long rmax = 0;
  if (any_res) {      // per residual member [r (n d) | dvec (n) | dloss/dr (n d) | dloss/ddvec (n)], freed when the call returns
    size_t tot = 0;
    for (int f = 0; f < F; ++f)
      if (sl.rho[f]) tot += 2 * ((size_t)p[f].n * p[f].d + p[f].n);
    FFGP_HIP(hipMalloc(&rbuf, tot * sizeof(double)));
    size_t off = 0;
    for (int f = 0; f < F; ++f) {
      if (!sl.rho[f]) continue;
      const long n = p[f].n, nd = n * p[f].d;
      rs.rho[f] = sl.rho[f];
      rs.yl[f] = r[f].y_low_dev; rs.yh[f] = r[f].y_high_dev;
      rs.vl[f] = r[f].v_low_dev; rs.vh[f] = r[f].v_high_dev; rs.vls[f] = r[f].v_low_stride; rs.vhs[f] = r[f].v_high_stride;
      rs.r[f] = rbuf + off; rs.dv[f] = rs.r[f] + nd;
      rs.gY[f] = rs.dv[f] + n; rs.gdv[f] = rs.gY[f] + nd;
      rs.rho_last[f] = r[f].rho_last_dev;
      rs.nd[f] = nd; rs.n[f] = (int)n; rs.nw[f] = sl.nw[f];
      off += 2 * (nd + n);
      rmax = std::max(rmax, std::max(nd, n));
      pq[f].Y_dev = rs.r[f];
      pq[f].diag_vec_dev = rs.vl[f] ? rs.dv[f] : nullptr;
      pq[f].diag_stride = 1;
    }
  }
  for (int f = 0; f < F; ++f) {
    memset(&g[f], 0, sizeof(ffgp_grads));
    g[f].g_w_dev = gbuf + (size_t)f * FFGP_TRAIN_GSTRIDE;
    g[f].g_amp_dev = g[f].g_w_dev + sl.nw[f];
    g[f].g_diag_add_dev = g[f].g_amp_dev + 1;
    if (sl.rho[f]) {
      g[f].g_Y_dev = const_cast<double*>(rs.gY[f]);
      if (rs.vl[f]) g[f].g_diag_vec_dev = const_cast<double*>(rs.gdv[f]);
    }
    all_small = all_small && ffgp_small_batch_ok(&pq[f], &g[f]);
  }
  p = pq.data();
  // the sticky status word starts clean: a failure of an EARLIER call on this handle is that call's to report
  if (const int zrc = ffgp_zero_async(h, h->d_info, 2 * sizeof(int))) {
    if (rbuf) hipFree(rbuf);
    return zrc;
  }
  // (the one-kernel paths -- n <= 40, or option small_finish -- apply the links inside their kernel and write raw gradients)
  const bool one_kernel = ffgp_small_ok(h, p, &g[0]) || ffgp_small2_ok(h, p, &g[0]);
  h->defer_info_copy = 1;      // (the per-call read-back of the status word: once, after the loop)
  h->fold_info = (F == 1) ? 1 : 0;   // one model: the Adam kernel clears / accumulates the status words (see ffgp_adam_kernel)
  int lrc = FFGP_OK;
  for (int k = 0; k < steps && lrc == FFGP_OK; ++k) {
    if (any_res) hipLaunchKernelGGL(ffgp_resid_form, dim3((unsigned)((rmax + 255) / 256), F), dim3(256), 0, h->stream, rs);
    if (all_small && F > 1) {
      if ((lrc = ffgp_zero_async(h, h->d_info, sizeof(int))) != FFGP_OK) break;
      if ((lrc = ffgp_small_batch_enqueue(h, F, p, lk.data(), loss, g.data())) != FFGP_OK) break;
      hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
    } else {
      for (int f = 0; f < F && lrc == FFGP_OK; ++f) lrc = nlml_fused_raw_enqueue(h, p + f, &lk[f], loss + f, &g[f]);
      if (lrc != FFGP_OK) break;
    }
    if (any_res) hipLaunchKernelGGL(ffgp_resid_grad, dim3(F), dim3(256), 0, h->stream, rs, gbuf);
    const double t = (double)(step0 + k + 1);
    const double bc1 = 1.0 - std::pow(opt->beta1, t), bc2 = 1.0 - std::pow(opt->beta2, t);
    hipLaunchKernelGGL(ffgp_adam_kernel, dim3(F), dim3(192), 0, h->stream, F, sl, gbuf, state_dev, state_stride, opt->lr, opt->beta1,
                       opt->beta2, opt->eps, bc1, std::sqrt(bc2), loss, trace_dev, trace_stride, k, h->d_info, h->fold_info,
                       (h->fold_info && !one_kernel) ? h->d_link + 256 : (const double*)nullptr, lk[0], p[0].D,
                       (lk[0].out_scale == 0.0) ? 1.0 : lk[0].out_scale);
  }
  h->defer_info_copy = 0;
  h->fold_info = 0;
  if (lrc != FFGP_OK) {
    hipStreamSynchronize(h->stream);
    if (rbuf) hipFree(rbuf);
    return lrc;
  }
  if (hipGetLastError() != hipSuccess) {
    hipStreamSynchronize(h->stream);
    if (rbuf) hipFree(rbuf);
    return FFGP_ERR_HIP;
  }
  FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ffgp_invalidate(h);
  const int rc = ffgp_wait(h);
  if (rbuf) hipFree(rbuf);
  return rc;
}

int ffgp_train_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, int steps, const ffgp_adam* opt, double* state_dev,
                   long state_stride, long step0, double* trace_dev, long trace_stride) {
  return train_impl(h, F, p, l, nullptr, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride);
}

int ffgp_train_residual_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* l, const ffgp_residual* r, int steps,
                            const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride) {
  if (!r) return FFGP_ERR_ARG;
  return train_impl(h, F, p, l, r, steps, opt, state_dev, state_stride, step0, trace_dev, trace_stride);
}

// copies a captured graph's staged outputs (value, then an optional gradient block) into the caller's buffers (the forward graph
// below)
__global__ void ffgp_rawg_copy_out(const double* __restrict__ stage, long len, double* __restrict__ nll, double* __restrict__ gbase) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) nll[0] = stage[0];
  if (t < len) gbase[t] = stage[1 + t];
}

// 40 < n <= 128 (one diagonal block): assemble and factor with the blocked path's kernels, then ONE finishing kernel (small.hip,
// FROM_FACTOR) for everything else -- links of the raw-parameter call included.  p holds the raw parameters when l is given.
static int small2_enqueue(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  FFGP_HIP(hipSetDevice(h->device));
  const int n = p->n, D = p->D;
  const size_t ld = ffgp_round_up(n, 16);
  FFGP_CHECK(ffgp_ensure_ws(h, (size_t)(n + 16) * ld * sizeof(double)));
  h->n_stages = 0;
  const double* w = p->w_dev;
  const double* amp = p->amp_dev;
  const double* dadd = p->diag_add_dev;
  if (l) {
    if (!h->d_link) FFGP_HIP(hipMalloc(&h->d_link, 512 * sizeof(double)));
    hipLaunchKernelGGL(ffgp_link_fwd, dim3(1), dim3(128), 0, h->stream, *l, D, p->w_dev, p->amp_dev, p->diag_add_dev, h->d_link);
    w = h->d_link;
    amp = h->d_link + D;
    if (dadd) dadd = h->d_link + D + 1;
  }
  FFGP_CHECK(ffgp_assemble_impl(h, p->X_dev, n, p->X_dev, n, D, w, amp, p->clamp_min, dadd, p->diag_vec_dev, p->diag_stride, p->add_mat_dev,
                                p->ld_add, p->add_all, p->mean_jitter, h->ws, (int)ld, 1, p->kfun, p->kparam));
  FFGP_CHECK(ffgp_potrf_impl(h, h->ws, n, n, (int)ld, 0));
  FFGP_CHECK(ffgp_small_enqueue(h, p, l, nll_dev, g, h->dinv));
  if (!h->fold_info) hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
  if (!h->defer_info_copy) FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return FFGP_OK;
}

static int nlml_fused_raw_enqueue(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* l, double* nll_dev, const ffgp_grads* g) {
  if (!h || !p || !l || !nll_dev) return FFGP_ERR_ARG;
  if (p->cov_dev || p->pair || p->tree || !p->w_dev || !p->amp_dev || p->D <= 0 || p->D > 128) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  if (p->n <= 0 || p->d <= 0 || !p->X_dev || !p->Y_dev || (p->ll_variant != FFGP_LL_V1 && p->ll_variant != FFGP_LL_V2)) return FFGP_ERR_ARG;
  if (!h->fold_info && ffgp_small_mfma_ok(h, p, g)) {   // n <= 128: ONE launch on the matrix cores (train.hip, evaluate mode) instead of the scalar one-workgroup
                                                        // kernel (n <= 40) or ~13 launches of the blocked path
    h->n_stages = 0;
    FFGP_CHECK(ffgp_zero_async(h, h->d_info, sizeof(int)));
    FFGP_CHECK(ffgp_small_mfma_enqueue(h, 1, p, l, nll_dev, g, 0));
    hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
    if (!h->defer_info_copy) FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ffgp_invalidate(h);
    return FFGP_OK;
  }
  if (ffgp_small_ok(h, p, g)) {   // one kernel: links, likelihood, gradients, chain rule, output scale
    h->n_stages = 0;
    FFGP_CHECK(ffgp_small_enqueue(h, p, l, nll_dev, g));
    if (!h->fold_info) hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
    if (!h->defer_info_copy) FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return FFGP_OK;
  }
  if (ffgp_small2_ok(h, p, g)) return small2_enqueue(h, p, l, nll_dev, g);
  if (!h->d_link) FFGP_HIP(hipMalloc(&h->d_link, 512 * sizeof(double)));
  const int D = p->D;
  double* eff = h->d_link;
  double* geff = h->d_link + 256;
  hipLaunchKernelGGL(ffgp_link_fwd, dim3(1), dim3(128), 0, h->stream, *l, D, p->w_dev, p->amp_dev, p->diag_add_dev, eff);
  ffgp_problem q = *p;
  q.w_dev = eff;
  q.amp_dev = eff + D;
  if (p->diag_add_dev) q.diag_add_dev = eff + D + 1;
  ffgp_grads gq;
  const ffgp_grads* gp = nullptr;
  bool chain = false;
  if (g) {
    gq = *g;
    if (g->g_w_dev) gq.g_w_dev = geff;
    if (g->g_amp_dev) gq.g_amp_dev = geff + D;
    if (g->g_diag_add_dev) gq.g_diag_add_dev = geff + D + 1;
    chain = g->g_w_dev || g->g_amp_dev || g->g_diag_add_dev;
    gp = &gq;
  }
  FFGP_CHECK(nlml_fused_enqueue(h, &q, nll_dev, gp));
  const double sc = (l->out_scale == 0.0) ? 1.0 : l->out_scale;
  if (chain && !h->fold_info)      // (ffgp_train_raw with one model: the Adam kernel applies the links' chain rule itself)
    hipLaunchKernelGGL(ffgp_link_bwd, dim3(1), dim3(128), 0, h->stream, *l, D, p->w_dev, p->amp_dev, p->diag_add_dev, geff, g->g_w_dev,
                       g->g_amp_dev, g->g_diag_add_dev, sc);
  if (sc != 1.0) {
    const long nY = (g && g->g_Y_dev) ? (long)p->n * p->d : 0, nv = (g && g->g_diag_vec_dev) ? p->n : 0;
    const long tot = nY > nv ? nY : nv;
    hipLaunchKernelGGL(ffgp_scale_outputs, dim3((unsigned)((tot > 0 ? tot : 1) + 255) / 256), dim3(256), 0, h->stream, sc, nll_dev,
                       g ? g->g_Y_dev : nullptr, nY, g ? g->g_diag_vec_dev : nullptr, nv, g ? g->g_kparam_dev : nullptr);
  }
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  return FFGP_OK;
}

// ---- the forward call as one captured graph (option "fwd_graph", default 0) ---------------------------------------------------
// A likelihood at N = 16384 is ~400 launches on two streams, issued by ONE host thread a few microseconds ahead of the GPU: on a busy
// host the step stretches (29 -> 35 ms was seen).  With the option on, the second identical forward-only call (same
// problem struct: same device buffers, sizes, options) is captured -- both streams: the side stream forks from and joins the capturing
// stream through the look-ahead's own events -- into a hipGraph that writes its value to a handle-owned slot, and from then on every
// such call is ONE hipGraphLaunch plus a one-word copy into the caller's output.  Same kernels, same order per stream, same values
// (test_forward_graph_replay); dropped with any option or buffer change.  Calls with gradients, with stage timing, or on the small-N
// paths are never captured.
// MEASURED (tools/host_load_probe.py, ROCm 7.2): idle host 28.65-29.02 ms launch by launch, 28.83-29.12 ms as a graph at N = 16384;
// 1.84 against 2.25-2.32 ms at N = 4096; with the pod's CPU quota exhausted by spinning processes both take exactly one cgroup period
// (100.0 ms) per step.  The runtime walks the graph's nodes on a host thread and issues them one by one: a graph does not take the host
// out of the step here.  What does help a multi-rank run is bench.py's per-rank CPU affinity.  Default off.
static int nlml_fused_plain(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g);

static int nlml_fused_enqueue(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g) {
  if (!h || !p || !nll_dev) return FFGP_ERR_ARG;
  const bool wants_grad = g && (g->g_w_dev || g->g_amp_dev || g->g_diag_add_dev || g->g_Y_dev || g->g_diag_vec_dev || g->g_cov_dev ||
                                g->g_kparam_dev || g->g_pair);
  const bool eligible = h->fwd_graph && !wants_grad && h->timing == 0 && p->n > FFGP_NB && !h->use_naive;
  if (!eligible) return nlml_fused_plain(h, p, nll_dev, g);
  if (!h->fwdg) {
    h->fwdg = new RawGraph();
    memset(h->fwdg, 0, sizeof(RawGraph));
  }
  RawGraph* r = h->fwdg;
  const bool same = (r->seen || r->valid) && !memcmp(&r->p, p, sizeof(ffgp_problem)) && r->epoch == h->alloc_epoch;
  FFGP_HIP(hipSetDevice(h->device));
  auto replay = [&]() -> int {
    FFGP_HIP(hipGraphLaunch(r->exec, h->stream));
    hipLaunchKernelGGL(ffgp_rawg_copy_out, dim3(1), dim3(256), 0, h->stream, r->stage, 0L, nll_dev, (double*)nullptr);
    ffgp_invalidate(h);     // the replay rewrote the handle's factor on the device; the host-side keys do not know
    h->graph_replays += 1;
    return hipGetLastError() == hipSuccess ? FFGP_OK : FFGP_ERR_HIP;
  };
  if (same && r->valid) return replay();
  if (!same) {              // first sight of this call: run it plainly (sizes every buffer, sets every kernel attribute), remember it
    rawg_drop_one(r);
    const int rc = nlml_fused_plain(h, p, nll_dev, g);
    r->p = *p;
    r->epoch = h->alloc_epoch;
    r->seen = (rc == FFGP_OK) ? 1 : 0;
    return rc;
  }
  if (!r->stage) {
    FFGP_HIP(hipMalloc(&r->stage, 2 * sizeof(double)));
  }
  r->seen = 0;
  if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return nlml_fused_plain(h, p, nll_dev, g);
  }
  const int rc = nlml_fused_plain(h, p, r->stage, nullptr);
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(h->stream, &graph);
  if (rc != FFGP_OK || ec != hipSuccess || !graph || r->epoch != h->alloc_epoch) {
    (void)hipGetLastError();
    if (graph) hipGraphDestroy(graph);
    if (getenv("FFGP_GRAPH_DEBUG")) fprintf(stderr, "[ffgp] forward graph: capture failed (rc %d, hip %d)\n", rc, (int)ec);
    return nlml_fused_plain(h, p, nll_dev, g);
  }
  hipGraphExec_t exec = nullptr;
  if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    hipGraphDestroy(graph);
    return nlml_fused_plain(h, p, nll_dev, g);
  }
  r->graph = graph;
  r->exec = exec;
  r->valid = true;
  return replay();
}

static int nlml_fused_plain(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g) {
  if (!h || !p || !nll_dev) return FFGP_ERR_ARG;
  const bool given_cov = (p->cov_dev != nullptr);
  if (p->n <= 0 || p->d <= 0 || !p->Y_dev) return FFGP_ERR_ARG;
  const bool pair = (!given_cov && (p->pair != nullptr || p->tree != nullptr));
  const ffgp_ktree pair2 = {2, FFGP_TREE_CHAIN, {p->pair_op, 0, 0}, p->pair};
  const ffgp_ktree* tree = p->tree ? p->tree : &pair2;
  if (pair && (tree->n_leaves < 2 || tree->n_leaves > 4 || !tree->leaf)) return FFGP_ERR_ARG;
  if (!given_cov && (p->D <= 0 || !p->X_dev)) return FFGP_ERR_ARG;
  if (!given_cov && !pair && (!p->w_dev || !p->amp_dev)) return FFGP_ERR_ARG;
  if (given_cov && p->ld_cov < p->n) return FFGP_ERR_ARG;
  if (p->ll_variant != FFGP_LL_V1 && p->ll_variant != FFGP_LL_V2) return FFGP_ERR_ARG;
  if (!pair && (p->kfun < FFGP_KFUN_SE || p->kfun > FFGP_KFUN_RQ)) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  const int n = p->n, D = given_cov ? 1 : p->D, d = p->d;
  const bool want_grad = g && (g->g_w_dev || g->g_amp_dev || g->g_diag_add_dev || g->g_Y_dev || g->g_diag_vec_dev || g->g_cov_dev ||
                                g->g_kparam_dev || (pair && g->g_pair));
  if (pair && g && (g->g_w_dev || g->g_amp_dev || g->g_kparam_dev)) return FFGP_ERR_ARG;   // a pair's kernel gradients travel in g_pair
  if (given_cov && g && (g->g_w_dev || g->g_amp_dev || g->g_kparam_dev)) return FFGP_ERR_ARG;
  if (g && g->g_cov_dev && g->ld_gcov < p->n) return FFGP_ERR_ARG;
  const bool v2 = (p->ll_variant == FFGP_LL_V2);
  const size_t ld = ffgp_round_up(n, 16);
  const size_t w0 = (size_t)(n + d) * ld;          // Sigma | Y^T  ->  L | Gamma^T
  const size_t n1 = ffgp_round_up((n + 1) / 2, FFGP_NB);
  size_t total = w0;
  size_t o_X = 0, o_S = 0, o_T = 0, o_At = 0, o_P = 0, o_A = 0, o_Ct = 0, o_Bt = 0;
  if (want_grad) {
    o_X = total; total += (size_t)n * ld;          // L^-1
    o_S = total; total += (size_t)n * ld;          // Sigma^-1 -> G
    o_T = total; total += 2 * (n1 * n1 + 16);      // TRTRI scratch + the top level's L21 X11 when the inverse is split
    o_At = total; total += (size_t)d * ld;         // A^T = (Sigma^-1 Y)^T
    o_P = total; total += (pair ? ffgp_grad_pair_partial_doubles(n, n, D, 0, tree->n_leaves) : ffgp_grad_partial_doubles(n, D)) + 16;
    if (v2) {
      o_Ct = total; total += (size_t)d * ld;       // (L^-1 A)^T
      o_Bt = total; total += (size_t)d * ld;       // B^T = (Sigma^-1 A)^T
    }
  }
  if (v2 && !want_grad) {
    o_A = total; total += (size_t)n * ffgp_round_up(d, 2) + 16;
  }
  if (ffgp_small_ok(h, p, g)) {   // the sizes of the reference's own demos: one workgroup, one launch (small.hip)
    h->n_stages = 0;
    FFGP_CHECK(ffgp_small_enqueue(h, p, nullptr, nll_dev, g));
    if (!h->fold_info) hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
    if (!h->defer_info_copy) FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return FFGP_OK;
  }
  if (ffgp_small2_ok(h, p, g)) return small2_enqueue(h, p, nullptr, nll_dev, g);
  FFGP_CHECK(ffgp_ensure_ws(h, total * sizeof(double)));
  double* W0 = h->ws;
  double* Gt = W0 + (size_t)n * ld;  // passenger rows: Gamma^T (d x n)

  h->n_stages = 0;
  stage_mark(h, 0);
  if (given_cov) {
    hipLaunchKernelGGL(ffgp_copy_lower_kernel, dim3((n + 31) / 32, (n + 31) / 32), dim3(256), 0, h->stream, p->cov_dev, p->ld_cov,
                       W0, (int)ld, n);
  } else if (pair) {
    FFGP_CHECK(ffgp_assemble_pair_impl(h, p->X_dev, n, p->X_dev, n, D, tree, p->diag_add_dev, p->diag_vec_dev,
                                       p->diag_stride, p->add_mat_dev, p->ld_add, p->add_all, p->mean_jitter, W0, (int)ld, 1));
  } else {
    FFGP_CHECK(ffgp_assemble_impl(h, p->X_dev, n, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, p->diag_add_dev,
                                  p->diag_vec_dev, p->diag_stride, p->add_mat_dev, p->ld_add, p->add_all, p->mean_jitter,
                                  W0, (int)ld, 1, p->kfun, p->kparam));
  }
  FFGP_CHECK(ffgp_transpose(h, p->Y_dev, n, d, d, Gt, (int)ld, 1.0));
  stage_mark(h, 1);
  // forward + gradients of a large block: the head of the triangular inverse (everything that only needs the factor's first n1s
  // columns: 3/4 of its flops) runs on a third stream under the factorisation's chain-bound tail
  int n1s = 0;
  if (want_grad && h->trtri_overlap && h->lookahead && !h->use_naive && n >= 4096 && n > h->la_min_n) {
    n1s = FFGP_NB;
    while (2 * n1s < n) n1s *= 2;
    if (n1s % h->nb_outer != 0) n1s = 0;
  }
  h->tri_hook_fired = 0;
  h->tri_hook_col = n1s;
  if (n1s) FFGP_CHECK(ensure_aux2(h));
  const int prc = ffgp_potrf_impl(h, W0, n, n + d, (int)ld, 0);
  h->tri_hook_col = 0;
  FFGP_CHECK(prc);
  const bool split_inv = n1s && h->tri_hook_fired;
  if (split_inv) {
    hipStream_t main_s = h->stream;
    FFGP_HIP(hipStreamWaitEvent(h->aux2, h->tri_ev[0], 0));
    h->stream = h->aux2;
    const int hrc = ffgp_trtri_head(h, W0, n, (int)ld, h->ws + o_X, (int)ld, h->ws + o_T, h->ws + o_T + n1 * n1 + 16, n1s);
    h->stream = main_s;
    FFGP_CHECK(hrc);
    FFGP_HIP(hipEventRecord(h->tri_ev[1], h->aux2));
  }
  stage_mark(h, 2);
  if (!v2) {
    FFGP_CHECK(ffgp_nll_reduce_impl(h, FFGP_LL_V1, W0, n, (int)ld, Gt, d, n, (int)ld, d, p->pi_const, nll_dev));
  } else if (!want_grad) {
    // A = L^-T Gamma  (n x d), then ||A||^2
    double* A = h->ws + o_A;
    const int lda2 = ffgp_round_up(d, 2);
    FFGP_CHECK(ffgp_transpose(h, Gt, d, n, (int)ld, A, lda2, 1.0));
    FFGP_CHECK(ffgp_trsm_lower_t_impl(h, W0, n, (int)ld, A, d, lda2));
    FFGP_CHECK(ffgp_nll_reduce_impl(h, FFGP_LL_V2, W0, n, (int)ld, A, n, d, lda2, d, p->pi_const, nll_dev));
  }
  stage_mark(h, 3);
  if (want_grad) {
    double* X = h->ws + o_X;
    double* S = h->ws + o_S;
    double* T = h->ws + o_T;
    double* At = h->ws + o_At;
    double* P = h->ws + o_P;
    if (split_inv) {
      FFGP_HIP(hipStreamWaitEvent(h->stream, h->tri_ev[1], 0));
      FFGP_CHECK(ffgp_trtri_tail(h, W0, n, (int)ld, X, (int)ld, T, T + n1 * n1 + 16, n1s));
    } else {
      FFGP_CHECK(ffgp_trtri_impl(h, W0, n, (int)ld, X, (int)ld, T));
    }
    stage_mark(h, 4);
    FFGP_CHECK(ffgp_lauum_impl(h, X, n, (int)ld, S, (int)ld));
    stage_mark(h, 5);
    // A^T = Gamma^T L^-1   (d x n)
    FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_MNMAJOR, TILES_FULL, 0, Gt, (int)ld, X, (int)ld, At, (int)ld, d, n, n, 1.0, 0.0,
                                TRI_LO_J));
    const double* gYt = At;  // V1: d nll / dY = A
    if (!v2) {
      // G = d/2 Sigma^-1 - 1/2 A A^T   (lower, in place of Sigma^-1)
      FFGP_CHECK(ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_LOWER, 0, At, (int)ld, At, (int)ld, S, (int)ld, n, n, d,
                                  -0.5, 0.5 * (double)d));
    } else {
      // V2 (Sigma^-2 quadratic form): value from ||A||^2; B = Sigma^-1 A = L^-T (L^-1 A);
      // G = d/2 Sigma^-1 - 1/2 (A B^T + B A^T);  d(-LL)/dY = B       
      double* Ct = h->ws + o_Ct;
      double* Bt = h->ws + o_Bt;
      FFGP_CHECK(ffgp_nll_reduce_impl(h, FFGP_LL_V2, W0, n, (int)ld, At, d, n, (int)ld, d, p->pi_const, nll_dev));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_KMAJOR, TILES_FULL, 0, At, (int)ld, X, (int)ld, Ct, (int)ld, d, n, n, 1.0, 0.0,
                                  TRI_HI_J));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_MNMAJOR, TILES_FULL, 0, Ct, (int)ld, X, (int)ld, Bt, (int)ld, d, n, n, 1.0,
                                  0.0, TRI_LO_J));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_LOWER, 0, At, (int)ld, Bt, (int)ld, S, (int)ld, n, n, d,
                                  -0.5, 0.5 * (double)d));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_MNMAJOR, OP_MNMAJOR, TILES_LOWER, 0, Bt, (int)ld, At, (int)ld, S, (int)ld, n, n, d,
                                  -0.5, 1.0));
      gYt = Bt;
    }
    FFGP_CHECK(ffgp_grad_impl(h, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, S, (int)ld, given_cov ? 0.0 : p->mean_jitter,
                              g->g_w_dev, g->g_amp_dev, g->g_diag_add_dev, g->g_diag_vec_dev, P, p->kfun, p->kparam,
                              g->g_kparam_dev));   // (a pair: only the trace / diagonal part runs here, tr G lands in d_scal[4])
    if (pair && g->g_pair)
      FFGP_CHECK(ffgp_grad_pair_impl(h, p->X_dev, n, p->X_dev, n, D, tree, S, (int)ld, 0, h->d_scal + 4,
                                     (p->mean_jitter != 0.0) ? p->mean_jitter / ((double)n * (double)n) : 0.0, P, g->g_pair));
    if (g->g_cov_dev)
      hipLaunchKernelGGL(ffgp_symmetrize_kernel, dim3((n + 31) / 32, (n + 31) / 32), dim3(256), 0, h->stream, S, (int)ld,
                         g->g_cov_dev, g->ld_gcov, n, 1.0);
    if (g->g_Y_dev) FFGP_CHECK(ffgp_transpose(h, gYt, d, n, (int)ld, g->g_Y_dev, d, 1.0));
    stage_mark(h, 6);
  }
  if (!h->fold_info) hipLaunchKernelGGL(ffgp_sticky_info_kernel, dim3(1), dim3(1), 0, h->stream, h->d_info);
  if (!h->defer_info_copy) FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return FFGP_OK;
}

// ------------------------------------------------------------------------------------------------------------
// posterior
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ffgp_var_diag_kernel(const double* __restrict__ Vt, int nt, int n, int ld,
                                                            const double* __restrict__ amp, double clamp, double add,
                                                            double* __restrict__ var, int kfun, double rinv) {
  // one wave per test point: var[t] = k(x*,x*) - sum_i Vt[t][i]^2 + add
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= nt) return;
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double v = Vt[(size_t)t * ld + i];
    s = __builtin_fma(v, v, s);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (lane == 0) var[t] = amp[0] * ffgp_kfun_val(kfun, rinv, fmax(0.0, clamp)) - s + add;
}

int ffgp_predict(ffgp_handle* h, const ffgp_problem* p, const double* Xs, int nt, int var_mode, double var_add_all,
                 double* mean_dev, double* var_dev, int ldv) {
  if (!h || !p || !Xs || nt <= 0 || !mean_dev) return FFGP_ERR_ARG;
  if (p->n <= 0 || p->D <= 0 || p->d <= 0 || !p->X_dev || !p->Y_dev || !p->w_dev || !p->amp_dev) return FFGP_ERR_ARG;
  FFGP_HIP(hipSetDevice(h->device));
  const int n = p->n, D = p->D, d = p->d;
  const size_t ld = ffgp_round_up(n, 16);
  const size_t total = (size_t)(n + d + nt) * ld;
  FFGP_CHECK(ffgp_ensure_ws(h, total * sizeof(double)));
  double* W0 = h->ws;
  double* Gt = W0 + (size_t)n * ld;        // Gamma^T (d x n)
  double* Vt = Gt + (size_t)d * ld;        // V^T = K_*^T L^-T (nt x n)
  h->n_stages = 0;
  stage_mark(h, 0);
  FFGP_CHECK(ffgp_assemble_impl(h, p->X_dev, n, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, p->diag_add_dev,
                                p->diag_vec_dev, p->diag_stride, p->add_mat_dev, p->ld_add, p->add_all, p->mean_jitter,
                                W0, (int)ld, 1, p->kfun, p->kparam));
  FFGP_CHECK(ffgp_transpose(h, p->Y_dev, n, d, d, Gt, (int)ld, 1.0));
  FFGP_CHECK(ffgp_assemble_impl(h, Xs, nt, p->X_dev, n, D, p->w_dev, p->amp_dev, p->clamp_min, nullptr, nullptr, 0, nullptr, 0,
                                0.0, 0.0, Vt, (int)ld, 0, p->kfun, p->kparam));
  stage_mark(h, 1);
  FFGP_CHECK(ffgp_potrf_impl(h, W0, n, n + d + nt, (int)ld, 0));
  stage_mark(h, 2);
  // mean = V^T Gamma   ([nt, n] x [n, d])
  FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_KMAJOR, TILES_FULL, 0, Vt, (int)ld, Gt, (int)ld, mean_dev, d, nt, d, n, 1.0, 0.0));
  if (var_dev) {
    if (var_mode == FFGP_VAR_FULL) {
      if (ldv < nt) return FFGP_ERR_ARG;
      FFGP_CHECK(ffgp_assemble_impl(h, Xs, nt, Xs, nt, D, p->w_dev, p->amp_dev, p->clamp_min, nullptr, nullptr, 0, nullptr, 0,
                                    var_add_all, 0.0, var_dev, ldv, 0, p->kfun, p->kparam));
      FFGP_CHECK(ffgp_gemm_launch(h, OP_KMAJOR, OP_KMAJOR, TILES_FULL, 0, Vt, (int)ld, Vt, (int)ld, var_dev, ldv, nt, nt, n, -1.0,
                                  1.0));
    } else {
      hipLaunchKernelGGL(ffgp_var_diag_kernel, dim3((nt + 3) / 4), dim3(256), 0, h->stream, Vt, nt, n, (int)ld, p->amp_dev,
                         p->clamp_min, var_add_all, var_dev, p->kfun, (p->kparam != 0.0) ? 1.0 / p->kparam : 1.0);
    }
  }
  stage_mark(h, 3);
  FFGP_HIP(hipMemcpyAsync(h->h_info, h->d_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  FFGP_HIP(hipStreamSynchronize(h->stream));
  stage_collect(h);
  return ffgp_map_info(h->h_info[0]);
}

// ------------------------------------------------------------------------------------------------------------
// instrumentation
// ------------------------------------------------------------------------------------------------------------
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

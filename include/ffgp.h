/*
 * libffgp -- MI355X (gfx950) native Gaussian-process hot path: C ABI.
 *
 * Drop-in boundary for the GP computation path of IceLab-X/FidelityFusion.  The reference has no FFI of its
 * own (it is pure Python on torch); each entry point below names the reference call it replaces
 * (file:line relative to the reference root).  The Python shim (fidelityfusion_amd/_lib.py, ctypes) is the
 * reference-side binding; INTEGRATION.md shows how the reference's modules would call it.
 *
 * Conventions
 *   - every pointer named *_dev is a DEVICE pointer to row-major (C-contiguous) fp64 data;
 *   - every call returns int: 0 = ok; > 0 = 1-based index of the first non-positive pivot (the matrix is not
 *     positive definite -- torch.linalg.cholesky raises torch.linalg.LinAlgError there); < 0 = FFGP_ERR_*;
 *   - work is enqueued on the handle's stream (ffgp_set_stream); calls that return a status derived from
 *     device data (ffgp_potrf, ffgp_nlml_fused, ffgp_predict) synchronise that stream before returning;
 *   - nothing here falls back to the CPU: without a gfx950 device ffgp_create fails;
 *   - THREADING: a handle owns mutable state (its stream binding, workspaces, the cached inverses) that calls modify while
 *     they run; at most ONE host thread may be inside a call on a given handle at any time.  Use one handle per thread
 *     (handles are cheap: two streams + workspaces grown on demand), or serialise calls on a shared one.
 *
 * Parameterisation.  All of the reference's stationary kernels on this path are
 *        K_ij = amp * exp(-1/2 * max(sum_k ((x_ik - x_jk) * w_k)^2, clamp_min))
 *   K1 ARDKernel               (GaussianProcess/kernel.py:88-105):   w = 1/(|length_scales|+1e-9), amp = |signal_variance|, clamp 1e-30
 *   K2 SquaredExponentialKernel(GaussianProcess/kernel.py:258-272):  w = exp(-length_scale) (all D), amp = exp(signal_variance)^2, clamp -inf
 *   K3 SE_kernel 2023          (MFGP_ver2023May/kernel/SE_kernel.py:20-44): w = 1/length_scale (or exp form), amp = scale
 * and every covariance on the path is
 *        Sigma = K + diag_add*I + diag(diag_vec) + add_mat + add_all*11^T + mean_jitter*mean(K)*I
 *   S1 cigp_v10.py:57-60           diag_add = exp(-log_beta)+1e-6, diag_vec = diag(y_var)
 *   S2 gp_computation_pack.py:125  diag_add = exp(-log_beta), mean_jitter = 1e-6
 *   S3 gp_basic.py:63-65,117-119   diag_add = noise_variance^2, add_mat = y_var
 *   S4 MFGP_ver2023May/base_gp/cigp.py:124-127  diag_add = 1e-6 + 1/noise, add_all = y_var
 * The raw->effective maps (abs, exp, pow) are O(D) and stay in the host language (torch autograd chains
 * through them); the ABI takes the effective w/amp/diag_add as DEVICE scalars so no call forces a D2H copy
 * of a parameter, and returns gradients with respect to those effective quantities.
 */
#ifndef FFGP_H
#define FFGP_H

#ifdef __cplusplus
extern "C" {
#endif

/* libffgp.so is linked with -fvisibility=hidden: exactly the functions declared in this header are exported
   (tests/test_abi_exports.py holds `nm -D` to this list, in both directions). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct ffgp_handle ffgp_handle;

enum {
  FFGP_OK = 0,
  FFGP_ERR_ARG = -1,    /* bad argument (null pointer, negative size, misaligned leading dimension) */
  FFGP_ERR_HIP = -2,    /* a HIP runtime call failed (message on stderr) */
  FFGP_ERR_ALLOC = -3,  /* device workspace allocation failed */
  FFGP_ERR_NODEVICE = -4,
  FFGP_ERR_HANDOFF = -5 /* a cross-stream hand-off of the factorisation's look-ahead never arrived and its gate gave up after option
                           "ho_timeout_ms" (a tool that serialises this process's kernels); the call's results are invalid */
};

/* likelihood formula variants */
enum {
  FFGP_LL_V1 = 1, /* nll = 1/2||L^-1 Y||^2 + d*sum(log L_ii) + 1/2*N*d*log(2*pi_const)
                     cigp_v10.py:61-69; gp_computation_pack.py:128-136; base_gp/cigp.py:129-136 (pi_const = 3.1415) */
  FFGP_LL_V2 = 2  /* -LL = 1/2(||Sigma^-1 Y||^2 + 2d*sum(log L_ii) + N*d*log(2*pi))  (the Sigma^-2 form of
                     Gaussian_log_likelihood 'cholesky3', gp_computation_pack.py:65-80; gp_basic.py:130-143) */
};

/* radial profile of the stationary kernel, K = amp * phi(s), s = max(||(x - x') o w||^2, clamp_min) */
enum {
  FFGP_KFUN_SE = 0,        /* phi = exp(-s/2)                                                 (K1, K2, K3) */
  FFGP_KFUN_MATERN12 = 1,  /* phi = exp(-sqrt(s)/rho)                       MaternKernel nu = 0.5, GaussianProcess/kernel.py:161-162 */
  FFGP_KFUN_MATERN32 = 2,  /* phi = (1 + a) exp(-a),          a = sqrt(3s)/rho           nu = 1.5, kernel.py:163-164 */
  FFGP_KFUN_MATERN52 = 3,  /* phi = (1 + a + a^2/3) exp(-a),  a = sqrt(5s)/rho           nu = 2.5, kernel.py:165-166 */
  FFGP_KFUN_RQ = 4,        /* phi = (1 + s/(2 alpha))^(-alpha), kparam = alpha (learnable: g_kparam)  RationalQuadraticKernel, kernel.py:297-310 */
  FFGP_KFUN_LINEAR = 5     /* not a radial profile: K = amp * sum_k w_k^2 (x_k - c_k)(x'_k - c_k)   LinearKernel, kernel.py:22-63.
                              Only valid inside an ffgp_kdesc (the two-descriptor entry points below) */
};

/* One part of a composed kernel -- SumKernel / ProductKernel, GaussianProcess/kernel.py:172-236; the reference's demos and
   two-fidelity models all run on SumKernel(LinearKernel, MaternKernel) (cigp_v10.py:81; two_fidelity_models/ResGP.py:25,
   AR_autoRegression.py:31, NAR_NonlinearAR.py:23).  Two descriptors + an operator are evaluated in ONE tile pass. */
typedef struct {
  int kfun;                  /* FFGP_KFUN_*  (FFGP_KFUN_LINEAR allowed) */
  const double* w_dev;       /* [D] inverse length scales */
  const double* amp_dev;     /* [1] amplitude */
  double clamp_min;          /* lower clamp on the squared distance (stationary parts) */
  double kparam;             /* rho / alpha of the profile */
  const double* center_dev;  /* [D] LinearKernel.center (FFGP_KFUN_LINEAR only; NULL = origin) */
} ffgp_kdesc;
typedef struct {             /* gradients w.r.t. one part's effective quantities; any pointer may be NULL */
  double* g_w_dev;           /* [D] */
  double* g_amp_dev;         /* [1] */
  double* g_kparam_dev;      /* [1] (FFGP_KFUN_RQ) */
  double* g_center_dev;      /* [D] (FFGP_KFUN_LINEAR) */
} ffgp_kdesc_grads;
enum { FFGP_KOP_SUM = 0, FFGP_KOP_PRODUCT = 1 };

/* A nested composition -- SumKernel / ProductKernel objects whose parts are themselves Sum / Product kernels (kernel.py:172-236
   compose arbitrary modules) -- with up to four leaves, evaluated in the same single tile pass.  Every binary tree with <= 4
   leaves is, up to the operand order of its (commutative, hence bit-identical) nodes, one of
       n_leaves = 2:  l0 op[0] l1
       n_leaves = 3:  (l0 op[0] l1) op[1] l2
       n_leaves = 4:  FFGP_TREE_CHAIN     ((l0 op[0] l1) op[1] l2) op[2] l3
                      FFGP_TREE_BALANCED  (l0 op[0] l1) op[2] (l2 op[1] l3)                                              */
enum { FFGP_TREE_CHAIN = 0, FFGP_TREE_BALANCED = 1 };
typedef struct {
  int n_leaves;              /* 2, 3 or 4 */
  int shape;                 /* FFGP_TREE_* (n_leaves = 4 only) */
  int op[3];                 /* FFGP_KOP_* of the n_leaves - 1 nodes, as numbered above */
  const ffgp_kdesc* leaf;    /* [n_leaves] */
} ffgp_ktree;

/* prediction outputs */
enum {
  FFGP_VAR_FULL = 0, /* cov[Nt,Nt] = K** - V^T V + var_add_all              (cigp_v10.py:41-44; gp_computation_pack.py:108-110) */
  FFGP_VAR_DIAG = 1  /* var[Nt]    = diag(K**) - colsum(V^2) + var_add_all  (base_gp/cigp.py:91-94) */
};

/* One GP block: inputs, targets, effective kernel/noise quantities.  All pointers are device pointers. */
typedef struct {
  int n;                  /* training points */
  int D;                  /* input dimension */
  int d;                  /* output columns */
  const double* X_dev;    /* [n, D] */
  const double* Y_dev;    /* [n, d] */
  const double* w_dev;    /* [D]  inverse length scales */
  const double* amp_dev;  /* [1]  amplitude */
  double clamp_min;       /* lower clamp on the squared distance (1e-30 for K1, -inf for K2/K3) */
  const double* diag_add_dev; /* [1] scalar added to the diagonal */
  const double* diag_vec_dev; /* optional: entry i at diag_vec_dev[i*diag_stride] (pass the N x N y_var with stride N+1) */
  long diag_stride;
  const double* add_mat_dev;  /* optional full [n, n] matrix added to Sigma (only its lower triangle is read) */
  int ld_add;
  double add_all;         /* scalar added to every entry */
  double mean_jitter;     /* coefficient of mean(K)*I (1e-6 for gp_computation_pack.negative_log_likelihood, else 0) */
  int ll_variant;         /* FFGP_LL_V1 | FFGP_LL_V2 */
  double pi_const;        /* 3.1415 for the V1 call sites, M_PI for V2 */
  int kfun;               /* FFGP_KFUN_* (0 = squared exponential) */
  double kparam;          /* rho of the Matern profiles (MaternKernel(rho=...), default 1); unused for SE */
  const double* cov_dev;  /* optional: a caller-built covariance [n, n] (lower triangle read).  When set, nothing is
                             assembled (X, w, amp, the diag and add fields are ignored) -- the Gaussian_log_likelihood(y, cov) call
                             shape of gp_computation_pack.py:34-91 -- and the gradient comes back through g_cov_dev */
  int ld_cov;
  const ffgp_kdesc* pair; /* optional: [2] descriptors of a composed kernel K = k[0] (+|x) k[1] on X_dev.  When set, w_dev / amp_dev /
                             clamp_min / kfun / kparam above are ignored and the kernel gradients come back through
                             ffgp_grads.g_pair; every Sigma extra (diag / matrix / all-entries / mean jitter) applies as usual.
                             Not accepted by ffgp_predict (the modules compose the posterior from ffgp_assemble_pair pieces). */
  int pair_op;            /* FFGP_KOP_SUM | FFGP_KOP_PRODUCT */
  const ffgp_ktree* tree; /* optional: a nested composition of 2-4 leaves in place of `pair` (same rules; ffgp_grads.g_pair then holds
                             n_leaves entries) */
} ffgp_problem;

/* Gradients of the value returned by ffgp_nlml_fused with respect to the effective quantities.
   Any pointer may be NULL (that gradient is skipped); all are device pointers. */
typedef struct {
  double* g_w_dev;        /* [D] */
  double* g_amp_dev;      /* [1] */
  double* g_diag_add_dev; /* [1]  (= tr G, plus the mean-jitter chain for S2) */
  double* g_Y_dev;        /* [n, d] */
  double* g_diag_vec_dev; /* [n]  (= diag G), optional */
  double* g_cov_dev;      /* [n, n] full symmetric d(value)/d(cov) (what torch's cholesky backward returns), optional */
  int ld_gcov;
  double* g_kparam_dev;   /* [1] d(value)/d(kparam) for FFGP_KFUN_RQ (alpha is an nn.Parameter, kernel.py:295), optional */
  const ffgp_kdesc_grads* g_pair; /* [2] gradients of the two parts when ffgp_problem.pair is set ([n_leaves] for .tree), optional */
} ffgp_grads;

/* ---- lifetime ------------------------------------------------------------------------------------------ */
int ffgp_create(int device, ffgp_handle** out);
int ffgp_destroy(ffgp_handle* h);
int ffgp_set_stream(ffgp_handle* h, void* hip_stream); /* hipStream_t; NULL restores the handle's own stream.  When the stream
                                                           changes, the new one is made to wait (event) for the work this handle
                                                           enqueued on the old one: the handle's workspaces are shared by both */
/* options: "timing" (0/1: record per-stage hipEvents; 2: also an event pair around every trailing-update launch),
            "nb_outer" (trailing-update block, multiple of 128; default 512),
            "naive" (1: route factor kernels through the slow reference kernels; debugging only),
            "lookahead" (default 1: factor panel k+1 on a high-priority side stream under the trailing update of step k),
            "la_min_n" (default 1024: smaller blocks are factored in order on one stream.  With event pairs between the two streams the
                        overlap did not pay for its hand-offs below ~3500 rows; with value hand-offs -- "ho_values" -- it does from two
                        panels on: N = 1280 / 1536 / 2048 / 2560 / 3072 / 3584 -3.4 / -2.1 / -4.3 / -4.2 / -5.0 / -6.1 %; 0 = look ahead at
                        every size),
            "la_carry" / "la_carry_n" / "la_carry_rows" (a panel's own update kernels also cover the next panel's first 128 columns, so
                        no strip update sits between two panels on the dependency chain: 1 = always, 0 = never (the S_a / S_b / S_ii
                        form), default 2 = throughout for blocks of at most la_carry_n rows (default 12288), and for larger blocks in
                        the ITERATIONS whose trailing matrix has at most la_carry_rows rows (default 8192): such a block starts in the
                        S_a / S_b / S_ii form -- there the chain hides under the update and the carry only widens its launches -- and
                        changes over.  Headline bench line, la_carry_rows = 0 / 6144 / 8192 / 10240 / 12288: 28.83 / 28.61 / 28.51 / 28.47 /
                        28.43 ms with the roofline kernel at 0.697 / 0.697 / 0.693 / 0.690 / 0.685 of peak beside the heavier chain),
            "ho_values" / "ho_defer" (default 1 / 2: the look-ahead's hand-offs between its two streams are values in device memory --
                        hipStreamWriteValue32 behind the producer, hipStreamWaitValue32 in front of the consumer, 2.9-4.7 us per hop
                        against 10.7-11.1 for hipEventRecord + hipStreamWaitEvent on this runtime -- and the word that says "panel k is
                        complete" is written by the next panel's first diagonal-block kernel as it starts instead of by a 5 us write
                        kernel on the chain: N = 4096 / 8192 / 12288 -5.3 / -2.4 / -1.7 %, values unchanged (ho_defer >= 1); with 2 the
                        hand-off of S_bz is likewise written by the S_ii launch behind it on the update stream: N = 16384 -0.4 %; ho_values = 0: the event
                        pairs, which are also what a stream under graph capture gets.  A value wait is a one-workgroup KERNEL that
                        polls the word, so a process whose kernels run strictly one at a time must not use it: ffgp_create starts a
                        handle with ho_values = 0 when it sees rocprofv3's counter collection (ROCPROF_COUNTER_COLLECTION: --pmc
                        serialises the dispatches of all queues), thread trace, the rocprofiler v1 / v2 tool libraries,
                        HIP_LAUNCH_BLOCKING or AMD_SERIALIZE_KERNEL in the environment; FFGP_HANDOFF=events / values overrides),
            "aux_prio" (default 1: raised wave priority for the side stream's kernels),
            "gemm_tile" (0 = automatic; 32 / 64 / 128 force the GEMM tile shape -- tests and benchmarks),
            "small_tile_threshold" (default 640: launches with fewer 128-tiles use 64-tiles),
            "tile32_threshold" (default 1024: K-major launches with fewer 64-tiles use 32-row tiles),
            "polite_m" (default 8192: trailing updates with fewer rows run one workgroup per CU so that the side
                        stream's kernels always find free registers and LDS; 6144 until the 128-tile staged its operands
                        directly into LDS -- a lone workgroup then ran at 0.82 of the MFMA cadence, now 0.88),
            "split_rem_max" (default 180: a 128-tile launch whose tile count leaves a remainder <= this modulo the 256 CUs
                        hands those last tiles out as 64 x 64 quarters -- same bits, a shorter last round; 0 = never),
            "syrk_light_tiles" (default 1: in the 128-tile symmetric updates a last tile row of at most 32 rows -- the passenger
                        rows of a likelihood with d <= 32 outputs -- runs as 16-row slabs, and the diagonal tiles run on the fast
                        tile's k loop without their strictly-upper quadrant -- same bits; 0 = general tiles for both),
            "super_block" / "super_min_n" (default 1024 / 2048: triangular sweeps on factors of at least super_min_n rows go
                        through inverted super_block x super_block diagonal blocks; 0 = always block by block),
            "skinny_max_n" (default 8: products with at most this many output columns run on the matrix-vector kernels; 0 = never),
            "splitk_min_k" (default 1024: products with <= 64 tiles of 64 x 64 and k >= this are cut along k; 0 = never),
            "asm_mm" / "asm_mm_min" / "asm_mm_grid" (default 1 / 6144 / 768: squared-exponential assemblies whose geometric-mean size
                        is at least asm_mm_min evaluate their interior 64 x 64 tiles on the matrix cores -- norm expansion, guarded
                        per 32 x 32 block by a fall-back to the difference form wherever a distance is below 1e-6 of the
                        squared norms -- with asm_mm_grid persistent workgroups; 0 = the difference kernel alone),
            "small_finish" (default 0; 1: 40 < n <= 128 runs assembly + blocked factorisation + ONE finishing kernel, 7 launches
                        instead of 21 -- measured +-5-10 % per training step),
            "trtri_fill" (default 0: the gradient path's triangular inverse, when its head runs under the factorisation, zeroes only the
                        diagonal blocks' upper parts of its N x N buffer -- every consumer reads it tile-wise below the diagonal;
                        1 = zero-fill the whole buffer first (2 GB per step at N = 16384; +0.2 ms); 2 = fill it with NaN, a test mode),
            "sb_lower" (default 1) / "sb_lower_min_n" (default 6144): for matrices of at least that many rows ffgp_syevd's band
                        reduction keeps only the LOWER triangle of the trailing matrix up to date (the rank-64 update is bound by
                        HBM: half the bytes) and forms A * Y from that triangle alone (every element serves the product and its
                        transpose); results agree with the full form to rounding.  n = 8192: update 21.8 -> 12.3 ms, A * Y and its
                        sums 16.1 -> 20.6 ms, eigh 234.3 -> 229.7 ms; below ~6000 rows the full form is as fast.  "sb_sym_wg"
                        (default 2048): workgroups the lower-triangle A * Y launch aims for,
            "chase_pack" (placement of the bulge chase's 256 working wavefronts: every pack-th workgroup works.  Default 1 = one per
                        compute unit over the whole chip (N = 8192: 64.6 ms; 2 = on every other XCD: 69.4, 4: 92, 8: 166); beside
                        other blocks' kernels 1 and 2 measure the same (config 5's eight blocks: 1.43-1.47 s per step either way),
            "fwd_graph" (default 0; 1 = forward-only likelihood calls of more than one diagonal block replay a captured hipGraph from
                        their second identical occurrence on: see ffgp_graph_replays -- measured, no gain on this runtime),
            "q2_split_min_cols" (default 8192: from this many columns of Z on, the eigensolver's back-transformation Z <- Q2 Z runs 32-column
                        slabs on eight waves -- ormq2 45.4 -> 38.9 ms at n = 8192, 434 -> 297 at 16384, values identical; below, the
                        slabs would not fill the chip),
            "polite64_pad_kb" (default 60, at most 64: unused dynamic LDS requested by the 64-tile trailing updates of ONE block's carry-form
                        look-ahead -- two of their workgroups per CU instead of four, so the chain's kernels are not slowed to a third
                        beside them; N = 4096 / 6144 / 8192 / 12288: -1.2 / -3.0 / -2.0 / -1.0 %, values unchanged; 0 = off),
            "polite32_pad_kb" (default 46: the same for that form's 32-tile trailing updates -- two workgroups per CU and room for the
                        chain's TRSM beside them: N = 3072 / 4096 / 5120 -1.0 / -0.8 / -0.5 % against 34 (three per CU), which had
                        been -0.8 ... -1.5 % against none; 0 = off),
            "diag_excl_rows" (default 4096: in the look-ahead's chain-bound iterations -- at most this many trailing rows -- a panel's first
                        diagonal-block kernel asks for a whole CU's LDS, so that the trailing-update workgroups it releases cannot land
                        beside it: N = 2048 / 4096 / 8192 -1.7 / -0.8 / -0.8 %, values unchanged; only while the handle is the process's
                        only one -- beside other handles' kernels an empty CU may be long in coming; 0 = never),
            "trsm128" / "trsm128_max_m" (default 1 / 8192: the factorisation chain's full-block TRSM runs on its own latency-shaped
                        kernel for panels of at most trsm128_max_m rows; the values are the general GEMM's bit for bit),
            "chase_xl" / "chase_xl_max_n" (default 1 / 2048: bands of up to chase_xl_max_n columns run their bulge chase with every
                        working wavefront on ONE XCD -- the kernel reads HW_REG_XCC_ID and the others leave -- and hand the band over
                        through that XCD's L2: plain stores, L1-bypassing loads; sb2st 7.9 -> 6.5 ms at n = 1024, 15.9 -> 13.8 at 2048;
                        0 = the chip-wide form with device-scope accesses at every size.  Where the runtime places a wave is observed
                        behaviour, not a contract: every XCD-local launch is followed by a chip-wide launch that chases whatever sweeps
                        the first did not hand out -- none on a full MI355X; all of them when no wave landed on the chosen XCD, as in a
                        partition mode or on a CU-masked stream),
            "ho_gate" / "ho_timeout_ms" (default 1 / 2000: the look-ahead's cross-stream waits are the library's own one-wave gate kernel,
                        which gives up after ho_timeout_ms without its value -- the call then returns FFGP_ERR_HANDOFF instead of hanging the
                        GPU, e.g. under a tool that runs this process's kernels one at a time and is not recognised at create time;
                        0 = hipStreamWaitValue32, which has no timeout),
            "ho_withhold" (test hook: k > 0 makes the k-th hand-off publication from now on never happen),
            "grad_lanes" (default 3: in ffgp_nlml_fused_batch, members of DIFFERENT sizes (all <= 6144 rows) run their inverse / gradient
                        stages side by side on up to three of the handle's streams, each with its own scratch; every member's launch
                        sequence is its single call's, so are its bits; 1 = member after member.  Measured -3 ... -6 %),
            "train_persist" (default 1: ffgp_train_raw runs sets of small models -- n <= 128, D, d <= 16 -- as ONE persistent kernel launch,
                        see ffgp_train_raw; 0 = one launch per stage and step, the round-5 form),
            "tlin_gemm_min" (default 8192: tensor-linear members of ffgp_train_tlin_raw with n l h >= this form y_low V^T and dloss/dV on
                        the fp64 MFMA GEMM, smaller ones in a plain fixed-order kernel -- faster up to n l h = 2048, slower from 14400 on,
                        profiles/train_tlin_bench.txt; 0 = never the GEMM),
            "chase_xcc" (0..15; default: handles of one process take XCDs 0..7 in turn -- the XCD whose wavefronts run the XCD-local
                        chase; a value no wave of the launch reports leaves the whole chase to the chip-wide launch behind it: a test mode),
            "batch_grad_ob" (default 1: the shared chain's gradient stage inverts all blocks in one outer-batched sequence of launches),
            "trtri_overlap", "small_fused", "small_max_n" (round-3 experiment switches).
   Retired keys, refused with FFGP_ERR_ARG like any unknown key: "raw_graph_max_n", "diag_dbg", "la_split", "nb_big", "nb_big_until",
   "sb_lookahead", "sb_av_gemm", "sb_qr4", "q2_wave4", "eig_overlap", "band_log2", "polite_pad_kb", "pass_split_min", "tail_mask_m",
   "tail_mask_cus", "syrk_h64", "syrk_direct" (switches of experiments that were measured and lost, docs/experiments.md; the library
   runs with the values they had by default), "diag_v2" and "diag_v4" (they chose among the diagonal-block kernels: the factorisation
   runs on ffgp_potrf_diag128_v4 -- two workgroup barriers per 16-column stage, 25.2 us per 128 x 128 block against 28.6 for round 4's
   flag-driven pipeline v3, forward N = 1024 / 4096 / 8192 -6.9 / -5.7 / -2.0 % -- and a factor produced elsewhere is inverted by
   ffgp_potrf_diag128; commit afe272f is the last tree with v3 and the barrier kernel's factor path).    */
int ffgp_set_option(ffgp_handle* h, const char* key, double value);
/* Create the handle's side streams now and use each once, so that they bind their hardware queues before streams the process creates
   later (ROCm binds at first use; a late stream shares a queue with an earlier one and runs in line with it).  For the main handle of
   a process that puts several blocks in flight on one GPU: call it before creating the worker streams.  No reference counterpart. */
int ffgp_prepare_streams(ffgp_handle* h);
const char* ffgp_version(void);
/* Always 0; kept for existing bindings. */
int ffgp_has_dev_options(void);
/* Number of forward calls this handle has served by replaying a captured graph since it was created (option "fwd_graph" of
   ffgp_set_option: the second identical forward-only call -- same problem struct, so the same device buffers; their CONTENTS may
   change -- is captured with both of its streams, later ones are one hipGraphLaunch and a one-word copy: same kernels, same values,
   the status of a failing pivot reported as by the plain call).  Measured on ROCm 7.2 (tools/host_load_probe.py): no gain -- this
   runtime executes a graph's nodes from a host thread one by one, so the step is 0.2-1 % slower at N = 16384, 22 % slower at
   N = 4096, and as exposed to a starved host as the plain launches; the option is off by default.  -1 for a NULL handle.  No reference
   counterpart. */
long ffgp_graph_replays(const ffgp_handle* h);

/* ---- building blocks ------------------------------------------------------------------------------------ */
/* K(x1,x2) [+ Sigma extras when the matrix is square and symmetric].  Replaces kernel.forward
   (GaussianProcess/kernel.py:88-105,258-272; MFGP_ver2023May/kernel/SE_kernel.py:20-44) and the torch.eye
   adds at cigp_v10.py:31-32,57-60; gp_computation_pack.py:125-126; gp_basic.py:63-65; base_gp/cigp.py:79-81,124-127.
   lower_only != 0: only tiles on/below the diagonal are written (n1 must equal n2).                      */
int ffgp_assemble(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D,
                  const double* w_dev, const double* amp_dev, double clamp_min, const double* diag_add_dev,
                  const double* diag_vec_dev, long diag_stride, const double* add_mat_dev, int ld_add,
                  double add_all, double mean_jitter, double* K_dev, int ldk, int lower_only, int kfun, double kparam);

/* The same for a composed kernel K = k[0] (+|x) k[1]  (k: two descriptors, op: FFGP_KOP_*): one write-only pass instead of
   the two kernel evaluations + elementwise combine + torch.eye adds of the reference (kernel.py:172-236 under
   cigp_v10.py:57-60).  Sigma extras as in ffgp_assemble.                                                        */
int ffgp_assemble_pair(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D, const ffgp_kdesc* k,
                       int op, const double* diag_add_dev, const double* diag_vec_dev, long diag_stride,
                       const double* add_mat_dev, int ld_add, double add_all, double mean_jitter, double* K_dev, int ldk,
                       int lower_only);
/* Backward of that call for a dense upstream dK [n1, n2]: g[e] = d sum(dK o K) / d{w, amp, kparam, center} of part e, one
   read of dK (autograd through Sum/ProductKernel.forward in the reference: two kernel backward chains).   */
int ffgp_kernel_grad_pair(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D, const ffgp_kdesc* k,
                          int op, const double* dK_dev, int ldk, const ffgp_kdesc_grads* g);

/* The same three calls for a nested composition (ffgp_ktree).  ffgp_kernel_input_weights_tree: for an upstream dK [n1, n2], leaf
   e's weight matrix lands at Wt_dev + e * leaf_stride (each [n1, ldw]):
       stationary leaf  Wt_e = dK o (d root / d leaf_e) o amp_e (-2 phi'_e):  dX1 = -w_e^2 o (rowsum(Wt_e) o X1 - Wt_e X2)
       linear leaf      Wt_e = dK o (d root / d leaf_e) o amp_e:              dX1 =  w_e^2 o (Wt_e (X2 - c_e))
   (autograd through Sum/ProductKernel.forward w.r.t. the inputs in the reference -- the acquisition loops of
   Bayesian_optimization/acq.py on the demo kernel SumKernel(LinearKernel, MaternKernel)).                         */
int ffgp_assemble_tree(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D, const ffgp_ktree* t,
                       const double* diag_add_dev, const double* diag_vec_dev, long diag_stride, const double* add_mat_dev,
                       int ld_add, double add_all, double mean_jitter, double* K_dev, int ldk, int lower_only);
int ffgp_kernel_grad_tree(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D, const ffgp_ktree* t,
                          const double* dK_dev, int ldk, const ffgp_kdesc_grads* g);
int ffgp_kernel_input_weights_tree(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D,
                                   const ffgp_ktree* t, const double* dK_dev, int ldk, double* Wt_dev, int ldw, long leaf_stride);

/* In-place lower Cholesky, A = L L^T (strictly-upper part is not referenced and not written).
   Replaces torch.linalg.cholesky at cigp_v10.py:35,61; gp_computation_pack.py:67,105,128; gp_basic.py:80,131;
   base_gp/cigp.py:83,129.  lda must be even and A_dev 16-byte aligned.                                     */
int ffgp_potrf(ffgp_handle* h, double* A_dev, int n, int lda);

/* Same factorisation with "passenger" rows: A is mtot x n (mtot >= n); the leading n x n block is factored and
   rows n..mtot-1 come out as A[n:, :] L^-T, i.e. (L^-1 B)^T for a right-hand side stored transposed below Sigma.
   This is how the fused paths obtain Gamma = L^-1 Y (cigp_v10.py:63) and V = L^-1 K_* (cigp_v10.py:36) inside
   the factorisation's own matrix-core GEMMs instead of separate triangular sweeps.                            */
int ffgp_potrf_rows(ffgp_handle* h, double* A_dev, int n, int mtot, int lda);

/* Backward of a standalone kernel evaluation: g_w[D], g_amp[1] = d sum(dK o K(x1,x2)) / d{w, amp} for a dense upstream
   dK [n1, n2] (autograd through kernel.forward when a caller builds its own Sigma, e.g. GaussianProcess/cigp_withMean.py:52). */
int ffgp_kernel_grad(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D,
                     const double* w_dev, const double* amp_dev, double clamp_min, int kfun, double kparam,
                     const double* dK_dev, int ldk, double* g_w_dev, double* g_amp_dev, double* g_kparam_dev);

/* Batched symmetric eigendecomposition of `batch` matrices M_b [n, n] (n <= 64; both triangles read), hand-written
 * two-sided cyclic Jacobi, one workgroup per matrix in LDS: Q_b's columns are the eigenvectors, evals_b the eigenvalues,
 * ascending (descending != 0: descending).  Replaces torch.linalg.eigh for the per-mode kernels of the HOGP block
 * (two_fidelity_models/hogp_simple.py:17-19,99-100) and is the inner solver of functional.eigh's blocked one-sided Jacobi.
 * Scale: every matrix is loaded times the power of two that brings its largest entry into [1, 2), and its eigenvalues are
 * multiplied back (both exact), so the convergence test and the rotations see the same image for M and for 2^k M.            */
int ffgp_syevj_small(ffgp_handle* h, const double* M_dev, int n, int ldm, int batch, long strideM, double* Q_dev, int ldq,
                     long strideQ, double* evals_dev, long strideE, int descending);

/* Batched symmetric eigendecomposition of `batch` matrices M_b [n, n] for 1 <= n <= FFGP_SYEV_LDS_MAX_N (the LOWER triangle is
 * read, as ffgp_syevd does; M is not modified): one workgroup per matrix, one launch, enqueued on the handle's stream only.  One
 * fp64 image of the matrix is all the CU's LDS holds at n = 128, so this is a one-sided (Hestenes) Jacobi on the positive definite
 * G = M + s I (s from Gershgorin's bound and the Frobenius norm): the orthogonalised, normalised columns are the eigenvectors and
 * the eigenvalues are their Rayleigh quotients against M.  Q_b's columns are the eigenvectors, evals_b the eigenvalues, ascending
 * (descending != 0: descending; ties by index as ffgp_syevj_small).  info_dev [batch] (may be NULL): 0 where matrix b converged,
 * else the number of column pairs its last sweep still rotated (every loop is bounded).  A NaN or Inf anywhere in the lower triangle
 * (or a row whose absolute sum overflows) gives NaN in every output of that matrix and info = n.
 * A zero matrix gives zeros and the identity.  FFGP_ERR_ARG, with nothing enqueued, for n outside 1..128, ldm < n, ldq < n or a
 * null M / Q / evals; batch <= 0 is FFGP_OK.  Replaces torch.linalg.eigh on the N x N input kernel of the HOGP block at the
 * reference's experiment sizes (two_fidelity_models/hogp_simple.py:15-19,97-100 on the 100 low-fidelity points of
 * Experiments/GAR_Aligned/exp_aligned.py:66-99), where ffgp_syevd's stage chain is dozens of launches and a host wait.          */
#define FFGP_SYEV_LDS_MAX_N 128
int ffgp_syev_lds(ffgp_handle* h, const double* M_dev, int n, int ldm, int batch, long strideM, double* Q_dev, int ldq,
                  long strideQ, double* evals_dev, long strideE, int descending, int* info_dev);

/* ---- symmetric eigensolver (the N x N `torch.linalg.eigh(K_x)` of the HOGP block) ------------------------------------------------
 * Full symmetric eigendecomposition A = Z diag(W) Z^T of a dense symmetric matrix (its LOWER triangle is read, as
 * torch.linalg.eigh's default UPLO does), eigenvalues ascending, eigenvectors in the COLUMNS of Z -- the contract of
 * `torch.linalg.eigh`, which the reference calls at two_fidelity_models/hogp_simple.py:15-19 (`eigen_pairs`), :97-100 (once per
 * likelihood evaluation on the N x N input kernel) and MFGP_ver2023May/base_gp/hogp.py:20-24.  Hand-written two-stage solver:
 * dense -> band (bandwidth 32; TSQR + Householder reconstruction per panel, rank-64 trailing updates on the fp64 matrix cores),
 * band -> tridiagonal (bulge chasing, one wavefront per sweep, pipelined through progress counters), tridiagonal divide &
 * conquer on the device (secular equation per root, Gu-Eisenstat vectors, merges as GEMMs), back-transformation with the
 * chase's reflectors (blocked WY on the matrix cores) and with the panels' (256-wide block reflectors, GEMMs).
 * n <= 32768 (workspace ~ 10 n^2 doubles).  A is not modified.  Synchronises the handle's stream before returning.
 * Scale contract: the solver is scale-covariant for finite A.  Every stage works on sigma A, sigma the power of two that brings the
 * largest |a_ij| of the lower triangle into [1, 2) (found on the device; 1 for the zero matrix), and W is multiplied by 1 / sigma
 * at the end; neither multiplication rounds, so ffgp_syevd(2^k A) returns exactly 2^k W and the same Z, bit for bit, as long as
 * no entry of sigma A or of the returned W falls into the denormal range.  Errors are relative to ||A||, whatever ||A|| is: entries
 * of 1e-160 or 1e150, whose squares are not representable, are solved as well as entries of order 1.  The rows and columns that
 * pad n to a multiple of 64 carry a diagonal of twice the largest absolute row sum of sigma A (1 for the zero matrix).  Only the
 * lower triangle decides sigma and the padding for n > 64; for n <= 64 (ffgp_syevj_small) both triangles are read.             */
int ffgp_syevd(ffgp_handle* h, const double* A_dev, int n, int lda, double* W_dev, double* Z_dev, int ldz);

/* The stages of ffgp_syevd on caller-owned buffers (n a multiple of 64, 64 <= n <= 32768) -- LAPACK's dsytrd_sy2sb / dsytrd_sb2st /
 * dstedc / dormtr split, exposed for tests, profiling and callers that want eigenvalues only:
 *   ffgp_sy2sb   A [n, n] full symmetric, DESTROYED -> AB [n, 64] band storage (element (r, c), 0 <= r - c <= 32, at AB[c * 64 + r - c])
 *                and Y [n, ldy]: the panels' unit-lower Householder blocks (panel p in columns 32p.., rows 32p + 32..; zero elsewhere)
 *   ffgp_sb2st   AB (destroyed) -> d [n], e [n] (e[n-1] = 0) and the chase's reflectors (refl: ffgp_sb2st_reflector_doubles(n) doubles)
 *   ffgp_stedc   (d, e) -> W [n] ascending, Z [n, ldz] eigenvectors of the tridiagonal matrix in columns.  Scale-covariant like
 *                ffgp_syevd: the divide and conquer runs on sigma d, sigma e with sigma the power of two that brings
 *                max(|d_i|, |e_i|) into [1, 2) -- its deflation tolerance (LAPACK dlaed2's) is one for a matrix of norm ~1, as in
 *                dstedc, which scales first -- and W is multiplied by 1 / sigma: ffgp_stedc(2^k d, 2^k e) = (2^k W, Z) exactly.
 *   ffgp_ormq2   Z[:, :ncols] <- Q2 Z   (the chase's reflectors);   ffgp_ormq1   Z[:, :ncols] <- Q1 Z   (the panels')
 * so that A = (Q1 Q2 Z) diag(W) (Q1 Q2 Z)^T.
 * ffgp_sy2sb and ffgp_sb2st do NOT scale: they form reflector norms from sums of squares, so the caller passes a matrix whose squared
 * entries neither underflow nor overflow (ffgp_syevd hands them its scaled image, entries of magnitude < 2).                      */
int ffgp_sy2sb(ffgp_handle* h, double* A_dev, int n, int lda, double* AB_dev, double* Y_dev, int ldy);
long ffgp_sb2st_reflector_doubles(int n);
int ffgp_sb2st(ffgp_handle* h, double* AB_dev, int n, double* d_dev, double* e_dev, double* refl_dev);
int ffgp_stedc(ffgp_handle* h, const double* d_dev, const double* e_dev, int n, double* W_dev, double* Z_dev, int ldz);
int ffgp_ormq2(ffgp_handle* h, const double* refl_dev, int n, double* Z_dev, int ldz, int ncols);
int ffgp_ormq1(ffgp_handle* h, const double* Y_dev, int ldy, int n, double* Z_dev, int ldz, int ncols);

/* ffgp_gemm over `batch` identical problems at fixed element strides (C_b = alpha op(A_b) op(B_b) + beta C_b). */
int ffgp_gemm_batched(ffgp_handle* h, int opa, int opb, int lower_tiles, const double* A_dev, int lda, long strideA,
                      const double* B_dev, int ldb, long strideB, double* C_dev, int ldc, long strideC, int m, int n, int k,
                      double alpha, double beta, int batch);

/* found_dev[i] = 1 iff row i of X1 [n1, D] equals (IEEE ==, element-wise) some row of X2 [n2, D]: the subset / unique-point
 * masks of the reference's data manager, `torch.all(x1.unsqueeze(1) == x2.unsqueeze(0), -1).any(-1)`
 * (FidelityFusion_Models/MF_data.py:196-199,234-237), as a device hash join instead of an N1 x N2 x D boolean temporary. */
int ffgp_rows_in(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D, unsigned char* found_dev);

/* Input gradients of a kernel call -- backward of `kernel(x1, x2)` w.r.t. x1 / x2, which the reference's autograd provides
 * and its acquisition optimisers rely on (Bayesian_optimization/acq.py:10-80 differentiate the posterior w.r.t. the test
 * points; CIGP_withMean.forward Bayesian_optimization/cigp.py:52-70).  For an upstream dK [n1, n2] writes
 *     Wt_ij = dK_ij * amp * (-2 phi'(s_ij))     (0 where the squared distance sits on the clamp)
 * so that dX1 = -w^2 o (rowsum(Wt) o X1 - Wt X2) and dX2 = -w^2 o (colsum(Wt) o X2 - Wt^T X1): two thin ffgp_gemm calls. */
int ffgp_kernel_input_weights(ffgp_handle* h, const double* X1_dev, int n1, const double* X2_dev, int n2, int D,
                              const double* w_dev, const double* amp_dev, double clamp_min, int kfun, double kparam,
                              const double* dK_dev, int ldk, double* Wt_dev, int ldw);

/* Rebuild the handle's store of inverted 128x128 diagonal blocks for a factor L that this handle did not just
   produce (the triangular solves and ffgp_potri consume it; ffgp_potrf leaves it up to date).
   CONTRACT of the cached inverses (ffgp_trsm_lower, ffgp_trsm_lower_t, ffgp_potrs, ffgp_potri): the store -- and the
   inverted super-blocks built on top of it -- is keyed on (L_dev, n, ldl) only.  A factor passed to those calls must be
   unmodified since the ffgp_potrf / ffgp_potrf_rows / ffgp_trtri_diag call ON THIS HANDLE that keyed the store.  If the
   contents at that address changed any other way (a buffer refilled by the caller, a factor written by another handle,
   a recycled allocation), call ffgp_trtri_diag again (or ffgp_invalidate) before solving with it.  ffgp_trtri_diag always
   rebuilds from block 0, whatever the store was keyed on before.
   One change needs no call: rows APPENDED below an unmodified leading factor at the same address and ldl (n grows, the
   first n_old rows are untouched) -- the next solve keeps the inverses of the complete leading blocks and builds the rest.  */
int ffgp_trtri_diag(ffgp_handle* h, const double* L_dev, int n, int ldl);

/* Drop the handle's cached inverses (diagonal blocks and super-blocks): the next triangular solve rebuilds them from
   the factor it is given.  Cheap; use it whenever a factor buffer is refilled behind the handle's back.        */
int ffgp_invalidate(ffgp_handle* h);

/* B <- L^-1 B.  Replaces torch.triangular_solve(B, L, upper=False) (cigp_v10.py:36,63;
   gp_computation_pack.py:130) and `L.inverse() @ B` (base_gp/cigp.py:131; gp_computation_pack.py:108).      */
int ffgp_trsm_lower(ffgp_handle* h, const double* L_dev, int n, int ldl, double* B_dev, int nrhs, int ldb);

/* B <- L^-T B (second half of cholesky_solve). */
int ffgp_trsm_lower_t(ffgp_handle* h, const double* L_dev, int n, int ldl, double* B_dev, int nrhs, int ldb);

/* B <- (L L^T)^-1 B.  Replaces torch.cholesky_solve (cigp_v10.py:39; gp_computation_pack.py:76,106). */
int ffgp_potrs(ffgp_handle* h, const double* L_dev, int n, int ldl, double* B_dev, int nrhs, int ldb);

/* out_dev[0] = 1/2*sum(M^2) + d*sum(log L_ii) + 1/2*n*d*log(2*pi_const)   (M = Gamma for V1, Sigma^-1 Y for V2 with
   the log-det counted as in FFGP_LL_V2).  Replaces cigp_v10.py:67-68 / gp_computation_pack.py:79.          */
int ffgp_nll_reduce(ffgp_handle* h, int variant, const double* L_dev, int n, int ldl, const double* M_dev, int d,
                    int ldm, double pi_const, double* out_dev);

/* Sinv (lower triangle) <- (L L^T)^-1 from the factor, via blocked TRTRI + LAUUM on the matrix cores. */
int ffgp_potri(ffgp_handle* h, double* L_dev, int n, int ldl);

/* C[m,n] = alpha * op(A) op(B) + beta * C on the fp64 matrix cores (the kernel under every O(N^3) stage).
   opa = 0: A stored m x k (k contiguous); opa = 1: A stored k x m (m contiguous), i.e. op(A) = A^T.
   opb = 0: B stored n x k (k contiguous), i.e. op(B) = B^T;  opb = 1: B stored k x n (n contiguous).
   lower_tiles != 0: only elements with col <= row are computed/written (m >= n, origin on the diagonal).
   tri: OR of 1 (k starts at the tile row), 2 (k starts at the tile column), 4 (k ends after the tile row),
        8 (k ends after the tile column) -- skips k-tiles that are structurally zero for triangular operands.
   Supported (opa, opb, lower_tiles): (0,0,*), (0,1,0), (1,0,0), (1,1,*).                                    */
int ffgp_gemm(ffgp_handle* h, int opa, int opb, int lower_tiles, int tri, const double* A_dev, int lda,
              const double* B_dev, int ldb, double* C_dev, int ldc, int m, int n, int k, double alpha, double beta);

/* ---- fused hot path ------------------------------------------------------------------------------------- */
/* nll_dev[0] <- negative log marginal likelihood of the block (V1: +nll; V2: -LL); if g != NULL also its
   closed-form gradients.  One call = assemble -> potrf -> trsm/potrs -> reduce (-> potri -> fused gradient).
   Replaces cigp.negative_log_likelihood (cigp_v10.py:50-69) + loss.backward() (FidelityFusion_Models/ResGP.py:84-87),
   gp_computation_pack.negative_log_likelihood (:120-136), GP_basic.log_likelihood (gp_basic.py:94-143),
   CIGP.compute_loss (MFGP_ver2023May/base_gp/cigp.py:99-136).  Returns 0, or the failing pivot index.       */
int ffgp_nlml_fused(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g);

/* The same call on RAW parameters: w_dev / amp_dev / diag_add_dev of the problem hold the module's own parameters and `links` names
   the elementwise maps to the effective quantities (the O(D) maps the reference's modules apply in torch: `abs() + eps` and the
   reciprocal of ARDKernel / MaternKernel, kernel.py:98,157; `exp` of SquaredExponentialKernel, :262-266; `exp(-log_beta)` of cigp,
   cigp_v10.py:57; `noise_variance ** 2` of GP_basic, gp_basic.py:63).  The maps and their chain rule run as two tiny kernels
   around the fused call, so a training step needs ONE library call instead of a dozen elementwise torch kernels and their
   autograd nodes -- which is what a step costs at the sizes the reference's own demos run (N = 16 ... 300).  Gradients in `g`
   come back with respect to the RAW parameters; with w_broadcast the single raw length scale feeds all D dimensions and g_w_dev
   receives ONE value.  D <= 128.                                                                                              */
enum {
  FFGP_LINK_ID = 0,           /* e = p                                                             */
  FFGP_LINK_INV_ABS_EPS = 1,  /* e = 1 / (|p| + c)                                                 */
  FFGP_LINK_EXP_NEG = 2,      /* e = exp(-p) + c                                                   */
  FFGP_LINK_INV = 3,          /* e = 1 / p + c                                                     */
  FFGP_LINK_ABS = 4,          /* e = |p|                                                           */
  FFGP_LINK_EXP_SQ = 5,       /* e = exp(p)^2                                                      */
  FFGP_LINK_SQUARE = 6        /* e = p^2 + c                                                       */
};
typedef struct {
  int w_link; double w_c; int w_broadcast;
  int amp_link; double amp_c;
  int dadd_link; double dadd_c;
  double out_scale;   /* the value and every gradient are multiplied by this (0 is read as 1): -1 turns the nll into the +LL the
                         reference's `negative_log_likelihood` returns (cigp_v10.py:69) without another elementwise kernel */
} ffgp_links;
int ffgp_nlml_fused_raw(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* links, double* nll_dev, const ffgp_grads* g);
/* the same call enqueued only: the status (a not-PD Sigma) is collected by the next ffgp_wait on this handle -- the Python modules
   issue a training step's likelihood this way and collect in backward(), so the host prepares the backward pass while the GPU works */
int ffgp_nlml_fused_raw_async(ffgp_handle* h, const ffgp_problem* p, const ffgp_links* links, double* nll_dev, const ffgp_grads* g);

/* F independent SMALL problems (n <= 128, D <= 16, d <= 16, one radial-profile kernel each, no caller-built covariance) in one
   launch per eight problems -- one workgroup each, everything in LDS: the per-fidelity / per-seed loops of the reference's
   experiments (Experiments/GAR_Aligned/exp_aligned.py:58-126; every model there has N = 16 ... 128) call cigp.negative_log_likelihood
   for one such model after the other.  p, g: arrays of F; links: array of F (raw parameters, as ffgp_nlml_fused_raw) or NULL
   (effective parameters); problem f's value lands in nll_dev[f].  The status is shared: a Sigma that is not positive definite in
   ANY member is reported (as that member's leading minor).  The _async form only enqueues (status: next ffgp_wait).
   Since round 6 problems within the one-launch trainer's limits (V1 likelihood, no add_mat / add_all / mean_jitter, no g_kparam) run on
   its matrix-core kernel (csrc/train.hip, evaluate mode: eight models per launch), as does ffgp_nlml_fused_raw at n <= 128; the others
   keep the scalar one-workgroup kernel.  Option "train_persist" = 0 restores the old routing.                                     */
int ffgp_nlml_fused_small_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, double* nll_dev,
                                const ffgp_grads* g);

/* F independent blocks (2 <= F <= 256; n > 128 each; V1 likelihood; one radial-profile kernel each) in one chain of launches: the
   per-fidelity / per-seed loops of the reference evaluate its blocks one after the other
   (Experiments/GAR_Aligned/exp_aligned.py:58-126, FidelityFusion_Models/ResGP.py:78-112), and below N ~ 6000 one block's
   factorisation is a latency-bound chain of short launches.  Here every launch of that chain covers all F blocks (diagonal-block
   kernel: one workgroup per block; GEMMs: the block index in gridDim.y), so the blocks share ONE chain; the arithmetic per block is
   the single call's, and the values are bit-identical to F separate calls.
   The blocks may have ONE shape (any n > 128) or DIFFERENT n and d (n <= 12288 each) -- the reference's fidelities are ragged:
   300 / 300 / 250 points in FidelityFusion_Models/ResGP.py:121-136, 100 low against 4..32 high in
   Experiments/GAR_Aligned/exp_aligned.py:66-74.  In a ragged batch every member follows the launch sequence of its own single call
   (in order up to "la_min_n" rows, the look-ahead's carry form above), launches of one kind at one chain step are merged with
   per-member sizes, and a member leaves the chain's launches when its columns are used up: the chain runs max(n) / 128 steps.
   p, g (may be NULL), links (NULL = effective parameters): arrays of F; nll_dev[f] receives block f's value; status[f] (host, may
   be NULL) its own factorisation status (0, or the 1-based index of the first non-positive pivot of THAT block).  Returns the first
   non-zero status; FFGP_ERR_ARG when the blocks do not meet the conditions -- also with option "naive" = 1, F > 256,
   a ragged member above 12288 rows -- and FFGP_ERR_ALLOC when the F-fold workspace does not fit: evaluate the blocks one by one
   (or in smaller batches) then, as fidelityfusion_amd/nlml.py::_chain_batches does.  Synchronous.                               */
int ffgp_nlml_fused_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, double* nll_dev,
                          const ffgp_grads* g, int* status);

/* K Adam training steps of F independent models (F <= 16) in ONE call -- the reference's hot loop
   (FidelityFusion_Models/ResGP.py:78-112; GaussianProcess/cigp_v10.py:92-104: per fidelity 100-1000 iterations of
   optimizer.zero_grad(); loss = -model.negative_log_likelihood(x, y); loss.backward(); optimizer.step() at N = 16 ... 500).
   p[f] / links[f] describe model f on its RAW parameters exactly as for ffgp_nlml_fused_raw (w_dev = raw length scales, amp_dev = raw
   signal variance, diag_add_dev = raw log_beta; links->out_scale = the sign that makes the value the loss to MINIMISE, +1 for
   loss = -negative_log_likelihood).  Per step: the likelihood and its closed-form gradients on the raw parameters (one launch for all
   models when every model is small -- the ffgp_nlml_fused_small_batch limits -- otherwise the launches of ffgp_nlml_fused_raw model
   after model), then one kernel that applies torch.optim.Adam's update (betas, eps, bias corrections as torch computes them; no
   weight decay, no amsgrad) to the three raw parameter tensors IN PLACE and stores the step's loss.  No host synchronisation inside
   the loop.  state_dev: per model [exp_avg (nw + 2) | exp_avg_sq (nw + 2)] at stride state_stride doubles (nw = 1 for a broadcast
   scalar length scale, else D; order: w, amp, diag_add), zero for a fresh optimiser and carried between calls together with step0 =
   the number of steps already taken; trace_dev[f * trace_stride + k] = loss of model f at step k, evaluated BEFORE that step's
   update (what the reference prints).  Returns 0, or the pivot status of the first step whose Sigma was not positive definite
   (torch.linalg.LinAlgError in the reference's loop): from that step on no parameter moves and the trace holds NaN.  Synchronous.
   ONE LAUNCH FOR THE WHOLE LOOP (round 6, csrc/train.hip): when every model has n <= 128, D <= 16, d <= 16, the V1 likelihood -- or the V2
   likelihood (GP_basic: ll_variant = FFGP_LL_V2 with diag_add under any link; V1 and V2 members of one call get a launch each) -- and no
   Sigma extra but diag_add / diag_vec -- what the reference's experiments run (Experiments/GAR_Aligned/exp_aligned.py:66-74: 100 low-
   against 4..32 high-fidelity points) -- the call is one kernel launch: a persistent workgroup per model keeps Sigma, its factor, the
   inverse, the parameters and the Adam moments in LDS and runs all `steps` iterations inside the kernel (option "train_persist" = 0
   restores the launch-per-stage loop).  There a failing model stops alone -- its trace holds NaN from its failing step on, its
   parameters are those it had when that step began -- while the other models of the call complete their steps; the return value is
   the first failing model's pivot status.  200 steps at n = 128: 9.7 ms (19.2 ms launch by launch); n = 32: 16 us per step. */
typedef struct ffgp_adam {
  double lr, beta1, beta2, eps;
} ffgp_adam;
int ffgp_train_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, int steps, const ffgp_adam* opt,
                   double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);

/* ffgp_train_raw with RESIDUAL members -- train_AR's fidelities above 0 (FidelityFusion_Models/AR_autoRegression.py:123-137): model f
   trains on the targets r = y_high - rho * y_low and, in the non-subset form, the diagonal extra dvec_i = |v_high,ii - rho * v_low,ii|
   (Sigma = K + diag_add + diag(dvec)), both re-formed from the current rho at every step and rounded as torch rounds
   `y_high - rho * y_low` (a product, then a difference).  rho is a fourth Adam parameter (same lr, betas, eps):
   dloss/drho = -sum_{i,q} A_iq y_low,iq - sum_i G_ii sgn(s_i) v_low,ii, with A = Sigma^-1 r, G = 1/2 (d Sigma^-1 - A A^T),
   s_i = v_high,ii - rho v_low,ii and sgn(0) = 0 (torch's abs backward).  r[f].rho_dev = NULL (or r = NULL) is a plain model, exactly as
   ffgp_train_raw trains it; plain and residual members may share a call.  For a residual member p[f].Y_dev and p[f].diag_vec_dev are
   ignored, and its Adam state is [exp_avg (nw + 3) | exp_avg_sq (nw + 3)] in the order w, amp, diag_add, rho.  rho_last_dev, when set,
   receives the rho at the start of the last step taken (what train_AR keeps as the fidelity's training data).  Everything else --
   routing (one launch for n <= 128, option "train_persist"), trace, status and failure semantics -- is ffgp_train_raw's.         */
typedef struct {
  double* rho_dev;            /* [1] raw rho, updated in place; NULL = a plain model */
  const double* y_low_dev;    /* [n, d] */
  const double* y_high_dev;   /* [n, d] */
  const double* v_low_dev;    /* optional: entry i at v_low_dev[i * v_low_stride] (pass an n x n var with stride n + 1) */
  long v_low_stride;
  const double* v_high_dev;   /* optional, set exactly when v_low_dev is */
  long v_high_stride;
  double* rho_last_dev;       /* optional [1] */
} ffgp_residual;
int ffgp_train_residual_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, const ffgp_residual* r, int steps,
                            const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);
int ffgp_nlml_fused_small_batch_async(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, double* nll_dev,
                                      const ffgp_grads* g);

/* ffgp_train_raw's ONE-LAUNCH form for WIDE-output models -- more than 16 target columns at n <= 128 (csrc/train_wide.hip): CIGAR's
   fidelity 0 on a field (FidelityFusion_Models/CIGAR.py:149-176: 128 points), ResGP and AR at Experiments/GAR_Aligned/exp_aligned.py's
   sizes (100 low- against 4..32 high-fidelity points, hundreds to thousands of columns).  The V1 likelihood and all its gradients see
   the targets only through inner products of their rows: with Z the stacked targets (Y of a plain member, [y_high; y_low] of a
   residual one; m = n or 2 n rows) any Z_eff [m, c] with Z_eff Z_eff^T = Z Z^T trains the same model, as long as the d of
   d sum log L_ii + n d / 2 log(2 pi) and of G = 1/2 (d Sigma^-1 - A A^T) stays the true one.  So the caller may pass the row blocks of
   U sqrt(max(Lambda, 0)) from the eigendecomposition of Z Z^T (c = m columns whatever d is) in place of the targets:
   p[f].d = the columns actually PASSED (Y_dev, or r[f].y_low_dev / y_high_dev: [n, p[f].d]), d_true[f] = the likelihood's d.
   A persistent workgroup per model factors Sigma once per step and then streams ceil(p[f].d / 16) column blocks through
   Gamma = L^-1 Y, A = L^-T Gamma, |Gamma|^2, sum A .* y_low and one MFMA group per owned block of A A^T; the gradient pass, the
   reduction and Adam are ffgp_train_raw's.  r may be NULL; r[f].rho_dev = NULL is a plain member; the member rules, the Adam state
   layout ([exp_avg (nw + 2) | exp_avg_sq (nw + 2)], a residual member nw + 3 with rho last), step0, the trace and rho_last_dev are
   ffgp_train_residual_raw's, so a state moves freely between the two calls; the two agree to rounding, not bit for bit.
   Covers F <= 16, n <= 128, D <= 16, d_true[f] > 16, p[f].d <= min(d_true[f], 128) for a plain member and min(d_true[f], 256) for a
   residual one, FFGP_KFUN_SE ... FFGP_KFUN_MATERN52, the V1 likelihood, diag_add and diag_vec.  FFGP_ERR_ARG, with nothing enqueued
   and nothing written, for anything else -- d_true[f] <= 16, n > 128, a tree, pair or caller-built covariance, the V2 likelihood,
   FFGP_KFUN_RQ, add_mat_dev, add_all, mean_jitter, a state_stride below the member's 2 (nw + 2 (+ 1)) -- which is never trained
   another way.  Failure semantics are the one-launch form's: a Sigma that is not positive definite stops that member alone at that
   step -- NaN in its trace from there on, its parameters, rho and moments as they were when the step began -- the others complete,
   and the call returns the pivot status of the first failing member in the caller's order, else 0.  info (host, may be NULL)
   receives every member's own status [F].  Synchronous.                                                                        */
int ffgp_train_wide_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, const ffgp_residual* r, const int* d_true,
                        int steps, const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev,
                        long trace_stride, int* info);

/* ffgp_train_raw with CAR members -- train_CAR's fidelities above 0 (FidelityFusion_Models/CAR_ContinuousAutoRegression.py:116-142):
   model f trains on the targets r = y_high - exp(b) * y_low (a product, then a difference, rounded as ffgp_train_residual_raw rounds
   its own) under the kernel kernel1(x, x') * s(b, l_z, sigma_z), the Monte-Carlo fidelity integral of fidelity_kernel_MCMC (:14-67)
   over the nz sample pairs (z1_i, z2_i).  With l = |l_z| + zeps and w2 = (hf - lf)^2:
       e_i = u_i - 1/2 ((z1_i - z2_i) / l)^2,   m = mean_i exp(e_i),   s = |sigma_z| m w2,
       u_i = fl32(fl32(fl32(-b) * fl32(z1_i - hf)) + fl32(fl32(-b) * fl32(z2_i - hf)))
   -- u_i in binary32 because torch evaluates `-b * (z1 - hf)`, a 0-dim fp64 parameter times an fp32 tensor, in binary32; z1 / l - z2 / l
   is two fp64 divisions of the widened samples; everything from exp on is fp64.  (Under torch.set_default_dtype(float64) the reference
   draws its samples in fp64 and nothing is binary32: pass those draws as z1d_dev / z2d_dev, and u_i = fl64(fl64(-b (z1_i - hf)) +
   fl64(-b (z2_i - hf))).)  The effective amplitude is link(amp_raw) * s; both
   the targets and s are re-formed from the current b, l_z, sigma_z at every step.  Six groups of parameters move per step (same lr,
   betas, eps): with T = dloss/d(effective amplitude),
       dloss/damp_raw = T s link'(amp_raw),       dloss/ds = T link(amp_raw),
       ds/dsigma_z = sgn(sigma_z) m w2,           ds/dl_z = |sigma_z| w2 sgn(l_z) mean_i[exp(e_i) (z1_i - z2_i)^2] / l^3,
       ds/db = -|sigma_z| w2 mean_i[exp(e_i) ((z1_i - hf) + (z2_i - hf))],
       dloss/db = dloss/ds * ds/db - exp(b) * sum(dloss/dr .* y_low)          (sgn(0) = 0; dloss/dr = A for V1, B for V2)
   and the derivatives of s in plain fp64 (the reference's ds/db is rounded to binary32 by autograd: 7e-8 relative, a documented
   deviation).  The base model's likelihood may be V1 or V2 (GP_basic gives V2).  c[f].b_dev = NULL is a plain model, exactly as
   ffgp_train_raw trains it; plain and CAR members may share a call.  For a CAR member p[f].Y_dev is ignored and its Adam state is
   [exp_avg (nw + 5) | exp_avg_sq (nw + 5)] in the order w, amp, diag_add, b, l_z, sigma_z.  b_last_dev, when set, receives the b at the
   start of the last step taken (train_CAR keeps y_high - exp(b) y_low at that b as the fidelity's data).  Routing: one launch for all
   steps when every member has n <= 128, D, d <= 16 (csrc/train.hip; V2 members included), else launch per stage -- before the
   likelihood a small kernel forms r and link(amp_raw) * s, after it another reduces dloss/db and applies the chain rule.  Trace,
   status, option "train_persist" and failure semantics are ffgp_train_raw's: in one-launch form a not-PD member stops alone and its
   parameters, b included, are those of the step's start.                                                                        */
typedef struct {
  double* b_dev;                 /* [1] raw b, updated in place; NULL = a plain model */
  double* zls_dev;               /* [1] raw length scale of the fidelity kernel */
  double* zamp_dev;              /* [1] raw signal variance of the fidelity kernel */
  double zeps;                   /* 1e-3 in the reference */
  const float* z1_dev;           /* [nz] the Monte-Carlo samples */
  const float* z2_dev;           /* [nz] */
  int nz;                        /* 1 .. 128 */
  double lf, hf;
  const double* y_low_dev;       /* [n, d] */
  const double* y_high_dev;      /* [n, d] */
  double* b_last_dev;            /* optional [1]: b at the start of the last step taken */
  const double* z1d_dev;         /* optional [nz] each: the samples as fp64 DRAWS (torch's default dtype set to float64: torch.rand */
  const double* z2d_dev;         /* then yields other numbers, not wider ones); z1_dev / z2_dev are ignored, u_i is fp64 arithmetic */
} ffgp_car_link;
int ffgp_train_car_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, const ffgp_car_link* c, int steps,
                       const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);

/* ffgp_train_raw with TENSOR-LINEAR members -- train_CIGAR's fidelities above 0 (FidelityFusion_Models/CIGAR.py:116-133): model f is a
   cigp trained on y_high - Tensor_linear(y_low), and the Tensor_linear's matrix sits under the same Adam as the three GP parameters.
   Only the LAST mode's matrix V [h, l] of a Tensor_linear acts (gp_computation_pack.py:155-158); with y_low [n, l], y_high [n, h = p.d]:
       targets     R = y_high - y_low V^T                       every entry one dot product over l in a fixed order, then one subtraction
       diag extra  |diag(v_high) - diag(v_low)|                  constant: the caller forms it once and passes it as p[f].diag_vec_dev;
                                                                 it does not depend on V and contributes nothing to V's gradient
       gradient    dloss/dV[a, b] = -sum_i (dloss/dR)[i, a] y_low[i, b],     dloss/dR = A = Sigma^-1 R (the V1 likelihood's g_Y_dev)
                                                                 every sum in a fixed order, no floating-point atomics
       Adam        V's h l entries are further Adam parameters (same lr, betas, eps, bias corrections): per member
                   [exp_avg (P) | exp_avg_sq (P)], P = nw + 2 + h l, in the order w, amp, diag_add, V row-major
   V is updated in place through its strides (Tensor_linear's bilinear initialisation for l < h is a transposed view).  t[f].V_dev =
   NULL is a plain model, trained exactly as ffgp_train_raw trains it; plain and tensor-linear members may share a call.  For a
   tensor-linear member p[f].Y_dev is ignored.  V_last_dev, when set, receives V (row-major) as it was at the start of the last step
   taken: train_CIGAR keeps y_high - Tensor_linear(y_low) at that V as the fidelity's data.
   ONE LAUNCH FOR THE WHOLE LOOP (csrc/train.hip, a class of members launched on its own as the CAR class is) when every member of the
   call has n <= 128, D <= 16, h <= 16 (so l <= 16) and what ffgp_train_raw's one-launch form asks besides: V, its two moments, dV and
   V as the step began stay in LDS for the whole call, R goes into the zero-padded target image and dV comes from A and y_low, both
   read from global memory at every step; everything else is ffgp_train_raw's step.  There a member whose Sigma is not positive
   definite stops alone: its trace holds NaN from that step on, and V, the moments and the three parameters keep the values they had
   when the step began (the factorisation comes first in the step: nothing of V has moved); the others complete.  Option
   "train_persist" = 0 restores the launch-per-stage loop.  Members with h > 16 always run launch per stage: V differs from column
   block to column block, so ffgp_train_wide_raw's Gram identity does not apply.
   LAUNCH PER STAGE at every other size: per step one launch forms every member's R into the call's buffer, the likelihood / gradient
   launches of ffgp_train_raw run with g_Y_dev set, one launch forms dV into a buffer of its own, and one launch -- a grid over the
   h l entries -- takes Adam's step (ffgp_train_raw's update function) on nw + 2 + h l values per member.  Members with
   n l h >= option "tlin_gemm_min" run both products on the fp64 MFMA GEMM (one launch each per member), smaller ones -- and a V with
   neither stride 1 -- in a plain fixed-order kernel.  No host synchronisation inside the loop.  There the status is shared by the
   call's members: from the first step whose Sigma was not positive definite in any member on nothing of the call moves (V and its
   moments included) and the trace holds NaN.  Trace, step0 and the return value are ffgp_train_raw's.
   FFGP_ERR_ARG, with nothing enqueued and nothing written: t == NULL, what ffgp_train_raw refuses, a tensor-linear member without
   y_low_dev / y_high_dev / X_dev, l outside 1..h (the reference only maps to an equal or finer output), a negative stride, the V2
   likelihood on such a member, state_stride < 2 P.  Synchronous.                                                               */
typedef struct {
  double* V_dev;              /* [h, l] raw, updated in place; NULL = a plain model */
  long V_row_stride;          /* element (a, b) of V at V_dev[a * V_row_stride + b * V_col_stride]; both 0 = row-major (l, 1) */
  long V_col_stride;
  int l;                      /* 1 .. h (h = p[f].d) */
  const double* y_low_dev;    /* [n, l] */
  const double* y_high_dev;   /* [n, h] */
  double* V_last_dev;         /* optional [h, l] row-major */
} ffgp_tlin_link;
int ffgp_train_tlin_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, const ffgp_tlin_link* t, int steps,
                        const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);

/* ffgp_train_raw for models whose kernel is a COMPOSITION -- SumKernel / ProductKernel trees of 2-4 leaves (ffgp_ktree), the kernel of
   the reference's own demos and of every two-fidelity model (SumKernel(LinearKernel, MaternKernel): GaussianProcess/cigp_v10.py:81,111,
   147; two_fidelity_models/ResGP.py:25,28) -- at every size, launch per stage.  p[f].tree describes model f (p[f].pair is not accepted
   here); the leaves' w_dev / amp_dev / center_dev and p[f].diag_add_dev hold the modules' RAW parameters, and links[f] names every
   leaf's maps as ffgp_links does for a single kernel (leaf[e] belongs to tree->leaf[e]; a FFGP_KFUN_LINEAR leaf with center_train has
   its centre trained as it stands, identity link).  Per step and without any host synchronisation: ONE launch maps all members' raw
   parameters to effective w [D], amp and diag_add in handle-owned scratch (ffgp_link_val's arithmetic: a leaf's values are those
   ffgp_nlml_fused_raw forms for a single kernel, bit for bit), the likelihood and its gradients run as ffgp_nlml_fused_async's own
   launches model after model on that scratch, and ONE launch applies the links' chain rule (a broadcast scalar length scale: its D
   effective gradients summed in index order, then one derivative), stores the losses in the trace and takes torch.optim.Adam's step
   on every raw parameter in place -- the update function of ffgp_train_raw's kernel.
   Adam state per model: [exp_avg (P) | exp_avg_sq (P)] at stride state_stride >= 2 P doubles, with
       P = sum over the leaves of (nw + 1 + (center_train ? D : 0)) + 1        (nw = 1 for a broadcast scalar length scale, else D)
   in the order leaf 0 (w, amp, centre), leaf 1, ..., then diag_add -- the tree's canonical leaf order.  Trace, state, step0, the
   return value and the failure semantics are ffgp_train_raw's launch-per-stage form: the status is shared by the call's members, and
   from the first step whose Sigma was not positive definite in ANY member on no parameter of the call moves and the trace holds NaN.
   Every Sigma extra and both likelihood variants of ffgp_nlml_fused's tree path are accepted.  FFGP_ERR_ARG, before anything is
   enqueued: F outside 1..16, a member without .tree or with n_leaves outside 2..4, a FFGP_KFUN_RQ leaf (its learnable alpha travels
   as a host double), cov_dev, D > 128, a leaf without w_dev / amp_dev, center_train on a leaf that is not linear or has no
   center_dev, state_stride < 2 P.  Synchronous.                                                                               */
typedef struct {
  int w_link; double w_c; int w_broadcast;   /* the leaf's raw w_dev holds 1 value (broadcast to all D) or D */
  int amp_link; double amp_c;
  int center_train;                          /* FFGP_KFUN_LINEAR: center_dev is a trained raw parameter [D] */
} ffgp_leaf_links;
typedef struct {
  ffgp_leaf_links leaf[4];
  int dadd_link; double dadd_c;
  double out_scale;                          /* as ffgp_links.out_scale (0 is read as 1) */
} ffgp_tree_links;
int ffgp_train_tree_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* links, int steps, const ffgp_adam* opt,
                        double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);

/* ffgp_train_tree_raw with RESIDUAL members -- train_AR's fidelities above 0 on a composed kernel (AR_autoRegression.py:123-137 with
   SumKernel(LinearKernel, MaternKernel), the kernel of two_fidelity_models/AR_autoRegression.py:31-37) -- launch per stage, at every
   size, both likelihood variants (csrc/train_tree_res.hip).  The arguments are ffgp_train_tree_raw's plus r, the struct and the member
   rules ffgp_train_residual_raw's: r == NULL or r[f].rho_dev == NULL makes model f a plain member, trained exactly as
   ffgp_train_tree_raw trains it (a call without any residual member IS ffgp_train_tree_raw's launches); for a residual member
   p[f].Y_dev and p[f].diag_vec_dev are ignored, it trains on r = y_high - rho * y_low (a product, then a difference, rounded as torch
   rounds it) and, in the non-subset form, on dvec_i = |v_high,ii - rho * v_low,ii|, both re-formed from the current rho at every step
   by ONE launch for all residual members into handle-owned scratch.  rho is one more Adam parameter:
       dloss/drho = -sum (dloss/dr) .* y_low - sum_i G_ii sgn(s_i) v_low,ii,      dloss/dr = A = Sigma^-1 r (V1), B = Sigma^-1 A (V2),
   sgn(0) = 0, reduced member by member in a fixed order inside the Adam launch (a member's trajectory does not depend on its
   companions), which then updates P + 1 parameters.  rho_last_dev receives the rho of the start of the last step taken.
   Adam state of a residual member: [exp_avg (P + 1) | exp_avg_sq (P + 1)] in the tree's canonical leaf order, then diag_add, then rho;
   state_stride >= 2 (P + 1), a plain member keeps 2 P.  FFGP_ERR_ARG, with nothing enqueued or written: what ffgp_train_tree_raw
   refuses, a state_stride below that, a residual member without y_low_dev / y_high_dev, v_low_dev set without v_high_dev (or the
   reverse), a negative variance stride.  Trace, status and failure semantics are ffgp_train_tree_raw's: the status is shared by the
   call, and from the first step whose Sigma was not positive definite in ANY member on no parameter (no rho either) moves.      */
int ffgp_train_tree_res_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* links, const ffgp_residual* r, int steps,
                            const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);

/* ffgp_train_tree_raw's job for SMALL members in ONE launch (csrc/train_tree_lds.hip): a persistent workgroup per model keeps Sigma,
   its factor, the raw parameters of every leaf and their Adam moments in LDS and runs all `steps` iterations inside the kernel, as
   ffgp_train_raw's one-launch form does for a single radial kernel.  The parameter list, the ffgp_problem / ffgp_tree_links
   description and the state layout -- [exp_avg (P) | exp_avg_sq (P)] in the canonical leaf order, stride state_stride >= 2 P -- are
   ffgp_train_tree_raw's, so one optimiser can be continued through either call; the arithmetic is not (the leaves are evaluated per
   entry from X and w^2, the factorisation is the LDS trainer's): the two agree to rounding, not bit for bit.
   Covers n <= 128, D <= 16, d <= 16, F <= 16, the V1 likelihood, diag_add and diag_vec, trees of 2-4 leaves in the FFGP_TREE_CHAIN /
   FFGP_TREE_BALANCED shapes with Sum / Product nodes, leaves FFGP_KFUN_SE ... FFGP_KFUN_MATERN52 (w_dev one broadcast value or D) and
   FFGP_KFUN_LINEAR (centre at the origin, given, or trained).  FFGP_ERR_ARG, with nothing enqueued and nothing written, for anything
   else: what ffgp_train_tree_raw refuses (a FFGP_KFUN_RQ leaf, n_leaves outside 2..4, F outside 1..16, ...), and n > 128, D > 16,
   d > 16, the V2 likelihood, add_mat_dev, add_all, mean_jitter.
   Return value and failure semantics are ffgp_train_raw's ONE-LAUNCH form, not ffgp_train_tree_raw's: a Sigma that is not positive
   definite stops that member alone at that step -- its trace holds NaN from there on, its parameters and moments the values they had
   when the step began -- the other members complete their steps, and the call returns the pivot status of the first failing member
   (in the caller's order), else 0.  Synchronous.                                                                              */
int ffgp_train_tree_lds_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* links, int steps, const ffgp_adam* opt,
                            double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);

/* ffgp_train_tree_lds_raw extended to the FFGP_LL_V2 likelihood and to RESIDUAL members (csrc/train_tree_lds_res.hip): ONE launch for
   all steps of the call's V1 members and one for its V2 members, a persistent workgroup per model.  Arguments and member rules are
   ffgp_train_tree_res_raw's (r == NULL or r[f].rho_dev == NULL: a plain member -- with r == NULL this is the way in for plain V2 tree
   models; ffgp_train_tree_lds_raw itself keeps its refusal of V2).  A residual member re-forms r = y_high - rho * y_low in the targets'
   LDS image and dvec = |v_high,ii - rho * v_low,ii| (the variances: two [128] rows in LDS) at the top of every step, and rho is
   parameter P of its Adam state [exp_avg (P + 1) | exp_avg_sq (P + 1)], interchangeable with ffgp_train_tree_res_raw's; rho_last_dev
   receives the rho of the start of the last step taken.  Coverage and failure semantics are ffgp_train_tree_lds_raw's: n <= 128,
   D <= 16, d <= 16, F <= 16, anything else FFGP_ERR_ARG with nothing enqueued or written; a member whose Sigma is not positive
   definite stops alone -- NaN in its trace from that step on, its parameters, rho and every moment as they were when the step
   began -- and the others complete.  Returns the pivot status of the first failing member in the caller's order, else 0.      */
int ffgp_train_tree_lds_res_raw(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* links, const ffgp_residual* r, int steps,
                                const ffgp_adam* opt, double* state_dev, long state_stride, long step0, double* trace_dev, long trace_stride);

/* K Adam steps of F <= 16 independent HOGP blocks in ONE call (csrc/train_hogp.hip) -- train_GAR's loop
   (FidelityFusion_Models/GAR.py:76-126: per fidelity 100-1000 iterations of HOGP_simple.log_likelihood / backward / Adam at 4..100
   points with 8 x 8 ... 64 x 64 outputs).  Launch per stage, no host synchronisation inside the loop, the status read once at the end.
   Model f: n points X_dev [n, D], targets Y_dev [n, d_1, ..., d_M] (M = nmodes in 1..3, every d_m <= 64, prod d_m <= FFGP_HOGP_MAX_OUT = 4096 -- two
   images of a sample's tensor live in LDS --, n <= FFGP_SYEV_LDS_MAX_N),
   ONE shared radial kernel on its raw parameters (w_dev: nw = 1 value with links.w_broadcast or D == 1, else D; amp_dev; kfun, kparam,
   clamp_min and links as for ffgp_train_raw -- dadd_link / dadd_c / out_scale are not read) and noise_dev [1], the raw
   noise_variance: tau = 1 / noise_variance, no jitter.  Mode m's inputs are the grid 0..d_m-1 as a float column, repeated in nw
   columns, formed by the call itself.  Per step, model by model (a model's arithmetic never depends on its companions):
     targets     a plain block uses Y_dev; a residual block r = y_high - y_low x_last V with the current V (a product, a difference)
     assembly    raw -> effective parameters (ffgp_link_val), K_0 [n, n] and K_1 ... K_M in one launch of ffgp_assemble's kernel
     eigenpairs  ffgp_syevj_small's kernel for n <= 64 and every mode matrix, ffgp_syev_lds's for 64 < n <= 128, ascending
     forward     A = ((lambda_0 lambda_1) ...) + tau, T_1 = Y x_m U_m^T, W = T_1 / A, g = W x_m U_m,
                 loss = (1/2 nd log 2 pi + 1/2 sum log A + 1/2 sum T_1 W) / nd          (nd = n prod d, the true pi)
     backward    dtau = 1/2 sum(1/A - W^2), c_m = the contraction of 1/A with the other modes' eigenvalues,
                 dK_m = 1/2 (U_m diag(c_m) U_m^T - g_(m) P_(m)^T), P = g x_{m' != m} K_m', everything times 1 / nd; dK_0 ... dK_M go
                 through ffgp_kernel_grad's kernels onto the effective parameters, the M + 1 contributions are summed (matrix 0 first),
                 then one link derivative each; d noise = -dtau / noise^2; a residual block: dV = -(g / nd contracted with y_low over
                 all but the last mode) [h, l]
     Adam        ffgp_adam_update on [w (nw) | amp | noise | V (h l, residual blocks only)]; the step's loss, evaluated before the
                 update, goes to trace_dev[f * trace_stride + k]
   Every sum has a fixed order (no floating-point atomics, no cross-workgroup waits), every loop is bounded.  The number of launches
   per step depends on M and on whether the block is residual, never on n or d_m.  The call's buffers live in the
   handle's workspace, kept between calls.  Everything is enqueued on the
   handle's stream except the eigensolvers, which are independent one-workgroup kernels: those of a step (all models') are dealt
   over the handle's stream and its two side streams, forked and joined by events, and the call returns with all three drained.
   Adam state per model at stride state_stride >= 2 P doubles, P = nw + 2 (+ h l): [exp_avg (P) | exp_avg_sq (P)]; step0[f] = the
   updates model f has already taken (its bias corrections use step0[f] + k + 1).
   Residual members (r != NULL and r[f].V_dev != NULL) are train_GAR's fidelities above 0: only the LAST mode's matrix of Tensor_linear
   acts (the reference applies every mode product to the input, gp_computation_pack.py:155-158), V_dev [h, l] is that matrix, raw,
   updated in place (strided: V_row_stride / V_col_stride; the Adam state and the trace see it row-major); y_low_dev [n, d_1, ..., d_{M-1}, l], y_high_dev [n, d_1, ..., d_{M-1}, h] with h = d_M; Y_dev is ignored.
   Caches (c may be NULL, as may any pointer in it): of the LAST step taken, i.e. for the parameters that step started from, K_m, their
   eigenvalues and eigenvectors (columns), A and g -- what HOGP_simple.forward reads.
   Failure: a model whose loss is not finite at some step (a non-positive entry of A after noise_variance crossed zero) or whose
   eigensolver reports a non-zero info stops alone: its trace holds NaN from that step on, its parameters and moments keep the values
   that step began with; the others complete.  fail_step (host, [F], may be NULL) receives the failing step of each model or -1.
   Returns 0, or 1 + f + 16 * k for the first failure (smallest step k, then smallest model f).  FFGP_ERR_ARG with nothing enqueued:
   F outside 1..16, n outside 1..128, nmodes outside 1..3, a dim outside 1..64, prod d_m > 4096, D outside 1..128, null buffers, a broadcast-link
   mismatch (w_broadcast != 0 names ONE raw value for D > 1 columns: with D == 1 it is refused), l outside 1..64, state_stride < 2 P, trace_stride < steps.  Synchronous. */
#define FFGP_HOGP_MAX_OUT 4096
typedef struct {
  int n, D;
  const double* X_dev;        /* [n, D] */
  int nmodes;                 /* 1 .. 3 */
  int dims[3];                /* each 1 .. 64, their product <= FFGP_HOGP_MAX_OUT */
  const double* Y_dev;        /* [n, d_1, ..., d_M]; ignored for a residual member */
  double* w_dev;              /* raw length scale(s), updated in place */
  double* amp_dev;            /* [1] raw signal variance, updated in place */
  double* noise_dev;          /* [1] raw noise_variance, updated in place */
  double clamp_min;
  int kfun;                   /* FFGP_KFUN_SE ... FFGP_KFUN_MATERN52 */
  double kparam;
} ffgp_hogp_model;
typedef struct {
  double* V_dev;              /* [h, l] raw, updated in place; NULL = a plain block */
  const double* y_low_dev;    /* [n, ..., l] */
  const double* y_high_dev;   /* [n, ..., h] */
  int l;                      /* 1 .. 64 */
  long V_row_stride;          /* element (a, b) of V at V_dev[a * V_row_stride + b * V_col_stride]; both 0 = row-major (l, 1). */
  long V_col_stride;          /* (Tensor_linear's bilinear initialisation is a transposed view: strides (1, h))               */
} ffgp_hogp_residual;
typedef struct {
  double* K_dev[4];           /* K_0 [n, n], K_m [d_m, d_m] */
  double* evals_dev[4];       /* ascending */
  double* evecs_dev[4];       /* columns */
  double* A_dev;              /* [n, d_1, ..., d_M] */
  double* g_dev;              /* [n, d_1, ..., d_M] */
} ffgp_hogp_cache;
int ffgp_train_hogp_raw(ffgp_handle* h, int F, const ffgp_hogp_model* m, const ffgp_links* links, const ffgp_hogp_residual* r, int steps,
                        const ffgp_adam* opt, double* state_dev, long state_stride, const long* step0, double* trace_dev,
                        long trace_stride, const ffgp_hogp_cache* c, int* fail_step);

/* K Adam steps of an ACQUISITION optimiser on a frozen posterior in ONE launch -- the reference's second hot loop
   (Bayesian_optimization/acq.py:48-68: `raw_samples` <= 500 query points, `num_restarts` = 30 iterations of zero_grad();
   loss = -acq(X).sum(); loss.backward(); Adam.step(), the model untouched).  The loss is a sum of per-point terms and Adam is
   element-wise: a workgroup owns 16 query points and runs all `steps` iterations on them without any cross-workgroup traffic
   (csrc/acq.hip), and a point's trajectory does not depend on which other points share the call.
   The posterior: training inputs X_dev [n, D], the Cholesky factor L_dev (ldl) of Sigma, alpha_dev [n] = Sigma^-1 y (d must be 1: an
   acquisition value is a scalar per point), ONE radial library kernel in its effective form (w_dev [D], amp_dev, clamp_min, kfun in
   FFGP_KFUN_SE ... FFGP_KFUN_RQ, kparam), var_add_all as in ffgp_predict.  L^-1 is formed once per call in handle workspace by the
   library's triangular inverse; the handle's inverted diagonal blocks are rebuilt from L_dev on every call (the result depends on the
   factor alone, not on what the handle served before) and are left keyed on L_dev, as after ffgp_trtri_diag.
   Per query point x: k = k(X, x), mean = k^T alpha, V = L^-1 k, var = amp - |V|^2 + var_add_all (phi(0) = 1), and
       FFGP_ACQ_UCB  a = mean + kappa sqrt(max(var, var_floor))        (no gradient through a variance below the floor: torch's clamp_min)
       FFGP_ACQ_EI   s = max(sqrt(var), 1e-9), u = mean - f_best - xi, Z = u / s, a = u Phi(Z) + s phi(Z)      (acq.py:161-181; Phi and
                     phi are constants of the reference's backward pass, which leaves da/dmean = Phi, da/ds = phi: the exact derivative)
   The loss is -sum a; its input gradient is ffgp_kernel_input_weights' formula with the upstream c_i = -(da/dmean alpha_i - 2 da/dvar B_i),
   B = L^-T V.  Adam is torch.optim.Adam's update as in ffgp_train_raw (bias corrections per step from step0, the steps already taken);
   state_dev [2, Q, D] = exp_avg | exp_avg_sq, zero for a fresh optimiser, carried between calls together with step0.
   Xq_dev [Q, D] is updated in place.  trace_dev [max(steps, 1), Q]: trace[k, j] = a_j at step k, BEFORE that step's update.  Optional:
   hist_dev [steps + 1, Q, D]: hist[k] = the points before step k, hist[steps] = the final points; grad_dev [Q, D] = the gradient of
   -sum a at the last evaluation.  steps = 0 is EVALUATE mode: trace[0] and grad_dev at Xq, nothing moves (opt / state_dev may be NULL).
   FFGP_ERR_ARG, before anything is enqueued (Xq, state and trace untouched): a null pointer, n outside 1..FFGP_ACQ_MAX_N, D outside
   1..FFGP_ACQ_MAX_D, steps outside 0..FFGP_ACQ_MAX_STEPS, d != 1, ldl < n, kfun = FFGP_KFUN_LINEAR or unknown, unknown acq, Q <= 0,
   step0 < 0.  Synchronous; returns 0 -- no factorisation runs inside, nothing in it can fail numerically.                         */
#define FFGP_ACQ_MAX_N 256        /* K_s, V and B of a 16-point tile stay in LDS as [n][16] images */
#define FFGP_ACQ_MAX_D 16
#define FFGP_ACQ_MAX_STEPS 4096
enum { FFGP_ACQ_UCB = 0, FFGP_ACQ_EI = 1 };
typedef struct {
  int n, D, d;
  const double* X_dev;
  const double* L_dev;
  int ldl;
  const double* alpha_dev;
  const double* w_dev;
  const double* amp_dev;
  double clamp_min;
  int kfun;
  double kparam;
  double var_add_all, var_floor;
  int acq;
  double kappa, xi, f_best;
} ffgp_acq_problem;
int ffgp_acq_optimize(ffgp_handle* h, const ffgp_acq_problem* p, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                      double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* The same loop on a STACK of frozen posteriors -- the multi-fidelity drivers' acquisition optimiser
   (MF_BayesianOptimization/Discrete/DMF_acq.py:226-262 on AR / ResGP / CAR: FidelityFusion_Models/AR_autoRegression.py:56-89) -- in
   ONE launch (csrc/acq_stack.hip).  Every member is a posterior as in ffgp_acq_problem, within that entry's limits, all of the same D;
   per query point q
       mean = sum_f on_f mean_coef_f (k_f^T alpha_f),   var = sum_f on_f var_coef_f (amp_f - |L_f^-1 k_f|^2 + var_add_all_f),
       on_f = (f <= level[q])      (level_dev NULL: every member; AR's `to_fidelity`, per point)
   and the acquisition value on (mean, var): FFGP_ACQ_UCB and FFGP_ACQ_EI exactly as ffgp_acq_optimize defines them, or
       FFGP_ACQ_UCB_VAR  a = mean + kappa var      (DMF_acq.py:49-63; this entry only)
   `level` enters as an exact 0 / 1 factor on a member's coefficients: a point's trajectory does not depend on its tile, its
   neighbours or their levels, and level = k everywhere is the stack cut after member k, bit for bit.  L_f^-1 of every member is
   formed once per call in handle workspace; the handle's inverted diagonal blocks are rebuilt before each and are left keyed on the
   LAST member's factor.  Xq, trace, hist, grad, step0, opt and evaluate mode (steps = 0) keep ffgp_acq_optimize's contract.
   state_dev is [2, Q, D] = exp_avg | exp_avg_sq, or with accumulate_grad [3, Q, D]: the third plane is the gradient accumulator --
   the driver's loop never calls zero_grad (DMF_acq.py:246-255), so the gradient Adam sees at step k is the sum of the gradients of
   steps 0..k; zero for a fresh optimiser, carried between calls like the moments.  grad_dev is the last evaluation's own gradient.
   FFGP_ERR_ARG, before anything is enqueued (Xq, state and trace untouched): a null pointer (level_dev, hist_dev and grad_dev may be
   NULL), F outside 1..FFGP_ACQ_MAX_MEMBERS, a member outside ffgp_acq_optimize's limits (n, D, d != 1, ldl < n or beyond int, kfun),
   members whose D differ, an unknown acq, Q <= 0, steps outside 0..FFGP_ACQ_MAX_STEPS, step0 < 0.  level values are read as
   min(level, F - 1); a negative level switches every member off.  Synchronous; returns 0.                                        */
#define FFGP_ACQ_MAX_MEMBERS 8
#define FFGP_ACQ_UCB_VAR 2   /* a = mean + kappa * var  (DMF_acq.py:49-63); stack entry only */
typedef struct {             /* one frozen member: the posterior fields of ffgp_acq_problem */
  int n, D, d;
  const double *X_dev, *L_dev; long ldl;
  const double *alpha_dev, *w_dev, *amp_dev;
  double clamp_min; int kfun; double kparam;
  double var_add_all;        /* this member's 1/beta */
  double mean_coef, var_coef;/* its weight in the stack's mean and variance (AR: rho, rho^2) */
} ffgp_acq_member;
typedef struct {
  int F; const ffgp_acq_member* members;   /* host array */
  const int* level_dev;      /* [Q] or NULL: point q sees members 0..level[q] (to_fidelity); NULL = all */
  double var_floor; int acq; double kappa, xi, f_best;
  int accumulate_grad;       /* 1: no zero_grad between steps, as DMF_acq.py:246-255 runs */
} ffgp_acq_stack;
int ffgp_acq_optimize_stack(ffgp_handle* h, const ffgp_acq_stack* s, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                            double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* ffgp_acq_optimize_stack past FFGP_ACQ_MAX_N training points: the same loop LAUNCH PER STAGE (csrc/acq_staged.hip), every step
   enqueued by this one call -- no host synchronisation and no Python inside the loop.  `s`, Xq, state, trace, hist, grad, step0, opt,
   evaluate mode (steps = 0), level, the coefficients, var_add_all, FFGP_ACQ_UCB / FFGP_ACQ_EI / FFGP_ACQ_UCB_VAR and accumulate_grad
   are ffgp_acq_optimize_stack's, field for field and layout for layout: an Adam state moves between the two entries, and a single
   posterior is the stack of one member with both coefficients 1.  Limits: every n in 1..FFGP_ACQ_STAGED_MAX_N; F, D, d = 1, steps and
   kfun as there.  Per call L_f^-1 of every member is formed in handle workspace (the handle's inverted diagonal blocks rebuilt from
   L_dev before each, left keyed on the LAST member's factor; only L's lower triangle within n columns is read) -- nothing is factored
   inside the loop.  Per step 5 + 2 F launches, whatever Q and n: K_s of all members, V_f = L_f^-1 K_s,f and B_f = L_f^-T V_f on the
   fp64 MFMA GEMM, column sums, the acquisition value, the input-gradient tiles, the owners' Adam update.  No atomics and no order of
   summation that depends on timing or on the grid: 12 + 18 steps through state_dev equal 30 steps bit for bit; cutting Q into several
   calls can change the GEMM's tile choice and with it the last bits.  The loop stops enqueueing at the first refused launch and
   returns that status.  FFGP_ERR_ARG, before anything is enqueued (Xq, state and trace untouched): everything
   ffgp_acq_optimize_stack refuses, with n outside 1..FFGP_ACQ_STAGED_MAX_N in place of its rule on n, and Q D beyond INT_MAX.
   Synchronous.
   Workspace, in doubles, with np_f = n_f rounded up to 16, Qp = Q rounded up to 64, C = the largest ceil(n_f / 128) and DM = 2, 8 or
   16 (the first that holds D):
       sum_f [ np_f^2  (L_f^-1)  +  4 n_f Qp  (K_s, its derivative factors, V, B)  +  n_f^2 / 4 + 128 n_f + 16  (triangular inverse) ]
       + F C Qp (2 + DM) + 3 Qp      (the chunk sums and the per-point values)
   -- 75 MiB for one member of 2048 points and Q = 500, 0.6 GiB for eight of them; a request the device cannot serve is FFGP_ERR_HIP.  */
#define FFGP_ACQ_STAGED_MAX_N 2048
int ffgp_acq_optimize_stack_staged(ffgp_handle* h, const ffgp_acq_stack* s, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                                   double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* The same loop on a CHAIN of frozen posteriors -- the drivers' acquisition optimiser on NAR (FidelityFusion_Models/NAR.py:30-61), whose
   upper fidelities take the lower fidelity's predicted MEAN as one more input column -- in ONE launch (csrc/acq_chain.hip).
   members[0] is a posterior on x [D], 1 <= D <= FFGP_ACQ_MAX_D - 1; members[f > 0] are posteriors on z = [x, m_{f-1}], D + 1 inputs;
   every member within ffgp_acq_optimize's limits otherwise.  Per query point x with s = min(level[q], F - 1) (level_dev NULL: F - 1):
       m_0 = k_0(X_0, x)^T alpha_0,    z_f = [x, m_{f-1}],  m_f = k_f(Z_f, z_f)^T alpha_f   for f = 1..s,
       mean = m_s,    var = amp_s - |L_s^-1 k_s(Z_s, z_s)|^2 + var_add_all_s
   -- the lower members contribute no variance, as NAR.forward discards cov_pred_low -- and the acquisition value on (mean, var):
   FFGP_ACQ_UCB, FFGP_ACQ_EI and FFGP_ACQ_UCB_VAR exactly as ffgp_acq_optimize_stack defines them.  The loss is -sum a; its gradient
   is taken through the whole chain (d m_f / d m_{f-1} included) and Adam acts on the D coordinates of x only.  Only the member a point
   stops at pays for the triangular chains; the others cost two O(n D) sweeps.  A point's trajectory does not depend on its tile, its
   neighbours or their levels, and level = k everywhere is the chain cut after member k, bit for bit.  Xq [Q, D], trace, hist, grad,
   step0, opt, evaluate mode (steps = 0), state_dev [2 | 3, Q, D] and accumulate_grad keep ffgp_acq_optimize_stack's contract, the
   workspace and the handle's inverted diagonal blocks likewise.  mean_coef / var_coef of a chain member are reserved and must be 1.0.
   FFGP_ERR_ARG, before anything is enqueued (Xq, state and trace untouched): everything ffgp_acq_optimize_stack refuses (its rule
   "members whose D differ" reads here: members[f > 0].D != members[0].D + 1), members[0].D outside 1..FFGP_ACQ_MAX_D - 1, a
   coefficient other than 1.  level values are read as min(level, F - 1); a point with a negative level stops at no member: its value
   is 0, its gradient 0 and it does not move.  Synchronous; returns 0.                                                            */
typedef struct {
  int F; const ffgp_acq_member* members;   /* host array; members[0].D = D, members[f>0].D = D + 1 */
  const int* level_dev;      /* [Q] or NULL = top */
  double var_floor; int acq; double kappa, xi, f_best;
  int accumulate_grad;
} ffgp_acq_chain;
int ffgp_acq_optimize_chain(ffgp_handle* h, const ffgp_acq_chain* c, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                            double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* ffgp_acq_optimize_chain past FFGP_ACQ_MAX_N training points: the same loop LAUNCH PER STAGE (csrc/acq_staged_chain.hip on the
   prologue and the shared stages of csrc/acq_staged.hip), every step enqueued by this one call -- NAR's own demo trains on 300 / 300 /
   250 points (FidelityFusion_Models/NAR.py:119-128).  The arguments are ffgp_acq_optimize_chain's, one for one, and so are the model,
   the outputs, the state layout [2 | 3, Q, D], accumulate_grad, the Adam arithmetic, evaluate mode (steps = 0) and the handling of
   level_dev (read as min(level, F - 1); a negative level stops at no member: value 0, gradient 0, the point does not move): an Adam
   state moves between the two entries.  Limits: every n in 1..FFGP_ACQ_STAGED_MAX_N; F <= FFGP_ACQ_MAX_MEMBERS, members[0].D in
   1..FFGP_ACQ_MAX_D - 1, members[f > 0].D = members[0].D + 1, d = 1, radial kfun, both coefficients 1.0, steps <= FFGP_ACQ_MAX_STEPS.
   Per call L_f^-1 of every member is formed in handle workspace as ffgp_acq_optimize_stack_staged forms it, and one small kernel over
   level_dev takes the census of the levels -- tops = the set of members at which some point stops, top = the highest of them --,
   read back once (4 bytes) before the step loop; with level_dev NULL tops = {F - 1} and nothing is read back.  Nothing is waited for
   inside the step loop.  The members of a chain run in sequence, so a step is, with the member index an argument of each launch:
       forward, f = 0..top:  K_s,f and its derivative factors on z_f = [x, m_{f-1}(x)] (the mean fed forward is the chunk sums added in
                             chunk order, the expression that reports it);  only for f in tops, V_f = L_f^-1 K_s,f and
                             B_f = L_f^-T V_f on the fp64 MFMA GEMM;  the column sums of K_s,f^T alpha_f and |V_f|^2
       the acquisition value on the mean and the variance amp_f - |V_f|^2 + var_add_all_f of the member each point stops at
       reverse, f = top..0:  the input-gradient tiles of member f -- upstream da/dmean alpha_i - 2 da/dvar B_iq for the points that stop
                             at f, -gu alpha_i for those that stop above it (gu = d(-a)/dm_f, member f + 1's partials of its last
                             input summed in chunk order), an exact 0 for the others
       the owners' sum over (member, chunk) of the D coordinates of x, the outputs and the Adam update
   -- 3 (top + 1) + 2 |tops| + 2 launches per step whatever Q and n: 13 for one level of a three-member chain.  No atomics and no
   order of summation that depends on Q, on timing or on the grid: a + b steps through state_dev equal a + b steps in one call bit for
   bit, and level = k everywhere is the chain cut after member k, bit for bit; cutting Q into several calls can change the GEMM's tile
   choice and with it the last bits.  The loop stops enqueueing at the first refused launch and returns that status.  FFGP_ERR_ARG,
   before anything is enqueued (Xq, state, trace, hist and grad untouched): everything ffgp_acq_optimize_chain refuses, with n outside
   1..FFGP_ACQ_STAGED_MAX_N in place of its rule on n, and Q D beyond INT_MAX.  Synchronous.
   Workspace, in doubles, with np_f, Qp and C as beside FFGP_ACQ_STAGED_MAX_N and DM = 2, 8 or 16 (the first that holds D + 1):
       sum_f [ np_f^2  (L_f^-1)  +  4 n_f Qp  (K_s, its derivative factors, V, B)  +  n_f^2 / 4 + 128 n_f + 16  (triangular inverse) ]
       + F C Qp (2 + DM) + 3 Qp  (the chunk sums and the per-point values)  + 1  (the census word)
   -- ffgp_acq_optimize_stack_staged's figure for the same members: 75 MiB for one member of 2048 points and Q = 500.               */
int ffgp_acq_optimize_chain_staged(ffgp_handle* h, const ffgp_acq_chain* c, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                                   double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* The single-posterior loop of ffgp_acq_optimize on a posterior whose kernel is a COMPOSITION -- the reference's own
   Bayesian-optimisation model runs on SumKernel(LinearKernel(1), MaternKernel(1)) (Bayesian_optimization/cigp.py:119; cigp_v10.py:81;
   two_fidelity_models/ResGP.py:25, AR_autoRegression.py:31) -- in ONE launch (csrc/acq_tree.hip).  `tree`: 2-4 leaves in the canonical
   forms of ffgp_ktree, every FFGP_KFUN_* profile, FFGP_KFUN_LINEAR (center_dev NULL = the origin) and FFGP_KFUN_RQ included; X_dev,
   L_dev (ldl), alpha_dev, d = 1 and var_add_all as in ffgp_acq_problem, within the same limits FFGP_ACQ_MAX_N / FFGP_ACQ_MAX_D /
   FFGP_ACQ_MAX_STEPS for every tree shape and leaf count.  Per query point x and training row i the leaves' values are
       radial:  v_e = amp_e phi_e(max(s_e, clamp_e)),  s_e = sum_k w_ek^2 (X_ik - x_k)^2        linear:  v_e = amp_e sum_k w_ek^2 (x_k - c_ek)(X_ik - c_ek)
   k_i = the tree on (v_e), its nodes rounded one by one as ffgp_assemble_tree rounds them; mean = k^T alpha, V = L^-1 k and
       var = k(x, x) - |V|^2 + var_add_all,    k(x, x) = the tree on the self values amp_e phi_e(max(0, clamp_e)) | amp_e sum_k w_ek^2 (x_k - c_ek)^2
   (a linear leaf makes k(x, x) depend on x: the loss gradient gains -(da/dvar) dk(x, x)/dx, as autograd through
   kernel(x, x).diagonal() gives it).  The input gradient is sum_i c_i sum_e (dk_i/dv_e) dv_e/dx with ffgp_acq_optimize's c_i, the
   dk/dv_e from the tree's reverse sweep, dv_e/dx = -amp_e (-2 phi_e') w_e^2 o (x - X_i) (zero where s_e < clamp_e) for a radial leaf
   and amp_e w_e^2 o (X_i - c_e) for a linear one.  acq: FFGP_ACQ_UCB or FFGP_ACQ_EI as defined there (FFGP_ACQ_UCB_VAR stays the
   stack entry's).  Xq, state [2, Q, D], trace, hist, grad, step0, opt and evaluate mode (steps = 0) keep ffgp_acq_optimize's contract;
   a point's trajectory does not depend on which other points share the call.
   FFGP_ERR_ARG, before anything is enqueued (Xq, state and trace untouched): a null pointer (tree, its leaf array and a leaf's w_dev /
   amp_dev included; hist_dev, grad_dev and a linear leaf's center_dev may be NULL), n_leaves outside 2..4, an unknown shape, op or
   leaf kfun, n outside 1..FFGP_ACQ_MAX_N, D outside 1..FFGP_ACQ_MAX_D, steps outside 0..FFGP_ACQ_MAX_STEPS, d != 1, ldl < n, acq not
   UCB or EI, Q <= 0, step0 < 0.  Synchronous; returns 0.                                                                         */
typedef struct {
  int n, D, d;
  const double* X_dev;
  const double* L_dev;
  int ldl;
  const double* alpha_dev;
  const ffgp_ktree* tree;
  double var_add_all, var_floor;
  int acq;
  double kappa, xi, f_best;
} ffgp_acq_tree_problem;
int ffgp_acq_optimize_tree(ffgp_handle* h, const ffgp_acq_tree_problem* p, double* Xq_dev, int Q, int steps, const ffgp_adam* opt,
                           double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* ffgp_acq_optimize_stack on a stack whose members may carry COMPOSED kernels -- the reference's two-fidelity AR and ResGP are built
   on SumKernel(LinearKernel(1), MaternKernel(1)) for both fidelities (two_fidelity_models/AR_autoRegression.py:31-34, ResGP.py:25-28),
   and its multi-fidelity models take any kernel_list -- in ONE launch (csrc/acq_stack_tree.hip).  `s` is ffgp_acq_stack as it stands;
   `trees` is a host array [s->F]:
       trees[f] == NULL   member f is one radial library kernel, taken from the member's own w_dev / amp_dev / clamp_min / kfun / kparam
                          exactly as ffgp_acq_optimize_stack reads them;
       trees[f] != NULL   member f's kernel is that tree of 2-4 leaves, with the canonical forms and per-leaf rules of
                          ffgp_acq_optimize_tree (FFGP_KFUN_LINEAR with optional center_dev, FFGP_KFUN_RQ); the member's own w_dev /
                          amp_dev / kfun are then not read and may be NULL / 0.
   Limits: F <= FFGP_ACQ_MAX_MEMBERS, every n <= FFGP_ACQ_MAX_N, one D <= FFGP_ACQ_MAX_D for all members, d = 1, steps <=
   FFGP_ACQ_MAX_STEPS.  Per query point q, with on_f = (f <= min(level[q], F - 1)) (level_dev NULL: every member),
       k_f,i = tree_f on the leaves' values at (X_f,i, x), its nodes rounded one by one as ffgp_assemble_tree rounds them,
       mean = sum_f on_f mean_coef_f k_f^T alpha_f,    var = sum_f on_f var_coef_f (k_f(x, x) - |L_f^-1 k_f|^2 + var_add_all_f),
       k_f(x, x) = tree_f on the self values amp_e phi_e(max(0, clamp_e)) | amp_e sum_k w_ek^2 (x_k - c_ek)^2;   a radial member: amp_f,
   and FFGP_ACQ_UCB, FFGP_ACQ_EI or FFGP_ACQ_UCB_VAR on (mean, var) as ffgp_acq_optimize_stack defines them.  The loss is -sum a; its
   gradient is the stack's -- the row sums with mean_coef_f alpha_f,i and var_coef_f B_f,i, combined as da/dmean Gm - 2 da/dvar Gv
   after the last member -- with each row's dk_i/dx from the tree's reverse sweep times the leaf derivative (ffgp_acq_optimize_tree's
   two forms, zero where s_e < clamp_e), plus the self term -da/dvar sum_f on_f var_coef_f dk_f(x, x)/dx, non-zero through linear
   leaves only.  on_f is an exact 0 / 1 factor on both coefficients: a point's trajectory does not depend on its tile, its neighbours
   or their levels, and level = k everywhere is the stack cut after member k, bit for bit.  accumulate_grad and state_dev [2 | 3, Q, D],
   Xq, trace, hist, grad, step0, opt, evaluate mode (steps = 0), the workspace and the handle's inverted diagonal blocks keep
   ffgp_acq_optimize_stack's contract (the members' leaf records travel in the same workspace, behind the bias corrections).
   FFGP_ERR_ARG, before anything is enqueued (Xq, state, trace, hist and grad untouched): everything ffgp_acq_optimize_stack refuses --
   its w_dev / amp_dev / kfun rules applying to the members with a NULL tree only --, trees NULL, and for a non-NULL tree what
   ffgp_acq_optimize_tree refuses about a tree: its leaf array NULL, n_leaves outside 2..4, an unknown shape, op or leaf kfun, a
   leaf's w_dev or amp_dev NULL.  Synchronous; returns 0.                                                                          */
int ffgp_acq_optimize_stack_tree(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, double* Xq_dev, int Q, int steps,
                                 const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* ffgp_acq_optimize_stack_tree past FFGP_ACQ_MAX_N training points: the same loop LAUNCH PER STAGE (csrc/acq_staged_tree.hip on the
   driver of csrc/acq_staged.hip), every step enqueued by this one call.  The arguments are ffgp_acq_optimize_stack_tree's, one for one
   (trees[f] == NULL: member f is one radial library kernel, read from the member's own fields), and so are the semantics, field for
   field and layout for layout: the per-point level, the coefficients, var_add_all, FFGP_ACQ_UCB / FFGP_ACQ_EI / FFGP_ACQ_UCB_VAR,
   accumulate_grad, evaluate mode (steps = 0), state_dev [2 | 3, Q, D], trace, hist and grad; k_f(x, x) is taken through the tree (a
   radial member: amp_f), and the loss gradient is da/dmean Gm - 2 da/dvar Gv - da/dvar S with S = sum_f on_f var_coef_f dk_f(x, x)/dx,
   non-zero through linear leaves only.  An Adam state moves between this entry, ffgp_acq_optimize_stack_tree, ffgp_acq_optimize_tree
   and ffgp_acq_optimize_stack_staged.  Limits: every n in 1..FFGP_ACQ_STAGED_MAX_N; F <= FFGP_ACQ_MAX_MEMBERS, one D <= FFGP_ACQ_MAX_D
   for all members, d = 1, steps <= FFGP_ACQ_MAX_STEPS.  Per call L_f^-1 of every member is formed in handle workspace and the leaf
   records are uploaded there, as ffgp_acq_optimize_stack_staged and ffgp_acq_optimize_stack_tree do.  Per step 5 + 2 F launches,
   whatever Q, n and the leaf counts: K_s of all members through their trees, V_f = L_f^-1 K_s,f and B_f = L_f^-T V_f on the fp64 MFMA
   GEMM, the column sums, the value (k_f(x, x), S and the acquisition), the input-gradient tiles -- which keep no derivative image: the
   leaves of a row are evaluated again and the tree's reverse sweep runs per row -- and the owners' Adam update.  No atomics and no
   order of summation that depends on timing or on the grid: a + b steps through state_dev equal a + b steps in one call bit for bit;
   cutting Q into several calls can change the GEMM's tile choice and with it the last bits.  The loop stops enqueueing at the first
   refused launch and returns that status.  FFGP_ERR_ARG, before anything is enqueued (Xq, state, trace, hist and grad untouched):
   everything ffgp_acq_optimize_stack_tree refuses, with n outside 1..FFGP_ACQ_STAGED_MAX_N in place of its rule on n, and Q D beyond
   INT_MAX.  Synchronous.
   Workspace, in doubles, with np_f, Qp, C and DM as beside FFGP_ACQ_STAGED_MAX_N:
       sum_f [ np_f^2  (L_f^-1)  +  3 n_f Qp  (K_s, V, B)  +  n_f^2 / 4 + 128 n_f + 16  (triangular inverse) ]
       + F C Qp (2 + DM) + 3 Qp  (the chunk sums and the per-point values)  + Qp DM  (S)  + 28 F  (the leaf records, 224 bytes each)
   -- 67 MiB for one member of 2048 points and Q = 500, 0.5 GiB for eight of them.                                              */
int ffgp_acq_optimize_stack_tree_staged(ffgp_handle* h, const ffgp_acq_stack* s, const ffgp_ktree* const* trees, double* Xq_dev, int Q,
                                        int steps, const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev,
                                        double* grad_dev);

/* ffgp_acq_optimize_chain on a chain whose members may carry COMPOSED kernels -- the reference's two-fidelity NAR is built on
   SumKernel(LinearKernel(1), MaternKernel(1)) below and SumKernel(LinearKernel(2), MaternKernel(2)) above
   (two_fidelity_models/NAR_NonlinearAR.py:23-26), and NAR(fidelity_num, kernel_list) takes any kernel list -- in ONE launch
   (csrc/acq_chain_tree.hip).  `c` is ffgp_acq_chain as it stands; `trees` is a host array [c->F]:
       trees[f] == NULL   member f is one radial library kernel, taken from the member's own w_dev / amp_dev / clamp_min / kfun / kparam
                          exactly as ffgp_acq_optimize_chain reads them;
       trees[f] != NULL   member f's kernel is that tree of 2-4 leaves, with the canonical forms and per-leaf rules of
                          ffgp_acq_optimize_tree (FFGP_KFUN_LINEAR with optional center_dev, FFGP_KFUN_RQ); the member's own w_dev /
                          amp_dev / kfun are then not read and may be NULL / 0.  Every leaf of member f carries D_f = members[f].D
                          weights -- D for f = 0, D + 1 above it, the last one on the mean fed forward -- and a centre of the same length.
   Limits, ffgp_acq_optimize_chain's: F <= FFGP_ACQ_MAX_MEMBERS, every n <= FFGP_ACQ_MAX_N, members[0].D = D in 1..FFGP_ACQ_MAX_D - 1,
   members[f > 0].D = D + 1, d = 1, both coefficients 1.0, steps <= FFGP_ACQ_MAX_STEPS.  Per query point x with
   s = min(level[q], F - 1) (level_dev NULL: F - 1), z_0 = x and z_f = [x, u], u = m_{f-1}:
       k_f,i = tree_f on the leaves' values at (Z_f,i, z_f), its nodes rounded one by one as ffgp_assemble_tree rounds them,
       m_f = sum_i alpha_f,i k_f,i   for f = 0..s,        mean = m_s,    var = k_s(z_s, z_s) - |L_s^-1 k_s|^2 + var_add_all_s,
       k_f(z, z) = tree_f on the self values amp_e phi_e(max(0, clamp_e)) | amp_e sum_k w_ek^2 (z_k - c_ek)^2;   a radial member: amp_f,
   and FFGP_ACQ_UCB, FFGP_ACQ_EI or FFGP_ACQ_UCB_VAR on (mean, var) as ffgp_acq_optimize_stack defines them; the lower members
   contribute no variance.  The loss is -sum a.  With t_i = -dk_f(Z_i, z)/dz over all D_f coordinates (the tree's reverse sweep times
   the leaf derivative, ffgp_acq_optimize_tree's two forms, zero where s_e < clamp_e), gm = da/dmean and gv = da/dvar:
       member s:       c_i = gm alpha_s,i - 2 gv B_i  (B = Sigma_s^-1 k_s),    G = sum_i c_i t_i[0..D),
                       gu = sum_i c_i t_i[D] - gv dk_s(z, z)/du,   dk_s(z, z)/du = sum over the linear leaves of
                            (dk_s(z, z)/dv_e) 2 amp_e w_e^2[D] (u - c_e[D])
       member f < s:   c_i = -gu alpha_f,i  (gu = d(-a)/dm_f),   G += sum_i c_i t_i[0..D),   the next gu = sum_i c_i t_i[D]
       d(-a)/dx = G - gv dk_s(z, z)/dx      (the self term: non-zero through linear leaves only, along x AND along u)
   -- in a chain a linear leaf sees the lower member's mean as an input coordinate, so the variance's self term feeds the chain as well.
   Adam acts on the D coordinates of x only.  Only the member a point stops at pays for the triangular chains and for k_f(z, z).  A
   chain without a linear leaf has both self terms exactly 0 and follows ffgp_acq_optimize_chain to rounding.  Switched-off members
   are selects that add exact zeros: a point's trajectory does not depend on its tile, its neighbours or their levels, and level = k
   everywhere is the chain cut after member k, bit for bit.  level values are read as min(level, F - 1); a point with a negative
   level stops at no member: its value is 0, its gradient 0 and it does not move.  Xq [Q, D], trace, hist, grad, step0, opt, evaluate
   mode (steps = 0), state_dev [2 | 3, Q, D] and accumulate_grad keep ffgp_acq_optimize_chain's contract -- an Adam state moves between
   this entry, ffgp_acq_optimize_chain and ffgp_acq_optimize_chain_staged --, the workspace and the handle's inverted diagonal blocks
   likewise (the members' leaf records travel in the same workspace, behind the bias corrections).
   FFGP_ERR_ARG, before anything is enqueued (Xq, state, trace, hist and grad untouched): everything ffgp_acq_optimize_chain refuses --
   its w_dev / amp_dev / kfun rules applying to the members with a NULL tree only --, trees NULL, and for a non-NULL tree what
   ffgp_acq_optimize_tree refuses about a tree: its leaf array NULL, n_leaves outside 2..4, an unknown shape, op or leaf kfun, a
   leaf's w_dev or amp_dev NULL.  Synchronous; returns 0.                                                                          */
int ffgp_acq_optimize_chain_tree(ffgp_handle* h, const ffgp_acq_chain* c, const ffgp_ktree* const* trees, double* Xq_dev, int Q, int steps,
                                 const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev, double* grad_dev);

/* ffgp_acq_optimize_chain_tree past FFGP_ACQ_MAX_N training points: the same loop LAUNCH PER STAGE (csrc/acq_staged_chain_tree.hip on
   the prologue and the shared stages of csrc/acq_staged.hip), every step enqueued by this one call -- the reference's NAR stands on
   SumKernel(LinearKernel, MaternKernel) fidelities (two_fidelity_models/NAR_NonlinearAR.py:23-26) and its demo trains on 300 / 300 /
   250 points (FidelityFusion_Models/NAR.py:119-128).  The arguments are ffgp_acq_optimize_chain_tree's, one for one (trees[f] == NULL:
   member f is one radial library kernel, read from the member's own fields), and so are the model, the outputs, the state layout
   [2 | 3, Q, D], accumulate_grad, the Adam arithmetic, evaluate mode (steps = 0) and the handling of level_dev (read as
   min(level, F - 1); a negative level stops at no member: value 0, gradient 0, the point does not move): an Adam state moves between
   this entry, ffgp_acq_optimize_chain_tree and ffgp_acq_optimize_chain_staged.  Limits, ffgp_acq_optimize_chain_staged's: every n in
   1..FFGP_ACQ_STAGED_MAX_N; F <= FFGP_ACQ_MAX_MEMBERS, members[0].D in 1..FFGP_ACQ_MAX_D - 1, members[f > 0].D = members[0].D + 1,
   d = 1, both coefficients 1.0, steps <= FFGP_ACQ_MAX_STEPS; a non-NULL tree as ffgp_acq_optimize_chain_tree accepts it.
   The step is ffgp_acq_optimize_chain_staged's -- the census of the levels once per call, the members in sequence,
   3 (top + 1) + 2 |tops| + 2 launches per step whatever Q and n -- with the stages of a composed kernel:
       forward, f = 0..top:  K_s,f = tree_f on the leaves' values at (Z_f,i, z_f), z_f = [x, m_{f-1}(x)] (the mean fed forward is the
                             chunk sums added in chunk order, the expression that reports it); only for f in tops the two GEMMs; the
                             column sums
       the value, per point with s = level:  k_s(z_s, z_s) through the tree on the self values, var = k_s(z, z) - |V_s|^2 +
                             var_add_all_s, the acquisition, and the self term's two shares S = dk_s(z, z)/dx and
                             su = dk_s(z, z)/du = sum over the linear leaves of (dk_s(z, z)/dv_e) 2 amp_e w_e^2[D] (u - c_e[D])
       reverse, f = top..0:  the input-gradient tiles of member f, which keep no derivative image (the leaves of a row are evaluated
                             again and the tree's reverse sweep runs per row); upstream gm alpha_i - 2 gv B_iq for the points that
                             stop at f, -gu alpha_i for those that stop above it, an exact 0 for the others;
                             gu = (member f + 1's partials of its last input summed in chunk order) - gv su when level = f + 1,
                             in that order
       the owners' sum over (member, chunk) of the D coordinates of x, minus gv S, the outputs and the Adam update.
   No atomics and no order of summation that depends on Q, on timing or on the grid: a + b steps through state_dev equal a + b steps
   in one call bit for bit, and level = k everywhere is the chain cut after member k, bit for bit; cutting Q into several calls can
   change the GEMM's tile choice and with it the last bits.  The loop stops enqueueing at the first refused launch and returns that
   status.  FFGP_ERR_ARG, before anything is enqueued (Xq, state, trace, hist and grad untouched): everything
   ffgp_acq_optimize_chain_tree refuses, with n outside 1..FFGP_ACQ_STAGED_MAX_N in place of its rule on n, and Q D beyond INT_MAX.
   Synchronous.
   Workspace, in doubles, with np_f, Qp and C as beside FFGP_ACQ_STAGED_MAX_N and DM = 2, 8 or 16 (the first that holds D + 1):
       sum_f [ np_f^2  (L_f^-1)  +  3 n_f Qp  (K_s, V, B)  +  n_f^2 / 4 + 128 n_f + 16  (triangular inverse) ]
       + F C Qp (2 + DM) + 3 Qp  (the chunk sums and the per-point values)  + Qp DM  (S)  + 28 F  (the leaf records, 224 bytes each)
       + 1 + Qp  (the census word, su)
   -- ffgp_acq_optimize_chain_staged's figure with three images per member instead of four.                                       */
int ffgp_acq_optimize_chain_tree_staged(ffgp_handle* h, const ffgp_acq_chain* c, const ffgp_ktree* const* trees, double* Xq_dev, int Q,
                                        int steps, const ffgp_adam* opt, double* state_dev, long step0, double* trace_dev, double* hist_dev,
                                        double* grad_dev);

/* Same, enqueue only: returns as soon as the work is on the handle's stream (nll/gradients are valid after
   ffgp_wait).  With one handle + stream per block, independent GP blocks (the fidelities of one model, the seeds
   of an experiment sweep) overlap on one GPU: one block's latency-bound factorisation tail runs under another
   block's trailing updates.                                                                                  */
int ffgp_nlml_fused_async(ffgp_handle* h, const ffgp_problem* p, double* nll_dev, const ffgp_grads* g);
/* Synchronise the handle's stream; returns the status of the last enqueued fused call (0 / failing pivot). */
int ffgp_wait(ffgp_handle* h);

/* Posterior at Xs[nt, D] for the block p (its ll_variant/pi_const are ignored; Sigma extras are honoured
   as given -- the reference's predict paths drop y_var, so callers pass the problem without it).
   mean_dev[nt, d] = K*^T Sigma^-1 Y;  var per var_mode with var_add_all added to every entry.
   Replaces cigp.forward (cigp_v10.py:24-48), conditional_Gaussian (gp_computation_pack.py:103-110),
   GP_basic.forward (gp_basic.py:78-84), CIGP.forward (base_gp/cigp.py:78-95).                               */
int ffgp_predict(ffgp_handle* h, const ffgp_problem* p, const double* Xs_dev, int nt, int var_mode,
                 double var_add_all, double* mean_dev, double* var_dev, int ldv);

/* The posteriors of F independent SMALL models at their own test points in ONE launch: what the reference's experiment drivers end with,
   one `gpr(x_train, y_train, x_test)` per fidelity, seed and training size (Experiments/GAR_Aligned/exp_aligned.py:63-107, ResGP.py:48-65,
   AR_autoRegression.py:56-89, CAR_ContinuousAutoRegression.py:94-114) -- after ffgp_train_raw the last per-model launch chain of a sweep.
   p[f] / links[f] describe model f exactly as for ffgp_nlml_fused_small_batch (raw parameters with links, or links == NULL for
   effective parameters); ll_variant and pi_const are ignored, as in ffgp_predict.  Limits per member: n <= FFGP_PREDICT_SMALL_MAX_N,
   D <= FFGP_PREDICT_SMALL_MAX_D, d <= FFGP_PREDICT_SMALL_MAX_d, one radial-profile kernel (kfun SE ... RQ with a constant kparam),
   diag_add as the only Sigma extra (no diag_vec / add_mat / add_all / mean_jitter, no caller-built covariance, no composed kernel: the
   reference's predict paths drop y_var).  1 <= F <= FFGP_PREDICT_SMALL_MAX_F.
   m[f]: the test points of model f and where its results go: mean_dev[nt, d] = K_s^T Sigma^-1 Y, var_dev[nt] = k(x, x) - colsum(V^2),
   V = L^-1 K_s, plus -- var_add_noise = 1 -- the value of the diag_add link WITHOUT its constant dadd_c (cigp.forward's 1/beta,
   cigp_v10.py:41-44, where Sigma carries 1/beta + jitter); 0 adds nothing (GP_basic.forward, gp_basic.py:78-84).
   The grid is (F, S): each of the S workgroups of a model factors it in LDS (the stages of the one-launch trainer, csrc/train_tile.h)
   and takes a fixed share of the model's tiles of 16 test points; S follows from F and the largest nt.  A point's mean and variance do not
   depend on S, on its tile or on the other points of the call, bit for bit.  (FFGP_PREDICT_SPLIT=k in the environment, read at every
   call, forces S = min(k, tiles): for tests.)
   A member whose Sigma is not positive definite stops alone: status[f] (host, may be NULL) = the 1-based index of its first non-positive
   pivot and its outputs are NaN; the others complete.  Returns the first non-zero status, or FFGP_ERR_ARG -- before anything is enqueued
   or written -- for null pointers, a member outside the limits, nt < 1 or F outside its range.  Synchronous.                          */
#define FFGP_PREDICT_SMALL_MAX_N 128
#define FFGP_PREDICT_SMALL_MAX_D 16
#define FFGP_PREDICT_SMALL_MAX_d 16
#define FFGP_PREDICT_SMALL_MAX_F 256
typedef struct ffgp_predict_member {
  const double* Xs_dev; int nt;      /* [nt, D] test points of THIS model */
  double* mean_dev;                  /* [nt, d] */
  double* var_dev;                   /* [nt]  diagonal variance */
  int var_add_noise;                 /* 1: add the diag_add link's value without its constant dadd_c; 0: add nothing */
} ffgp_predict_member;
int ffgp_predict_small_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_links* links, const ffgp_predict_member* m,
                             int* status);

/* ffgp_predict_small_batch for members on a COMPOSED kernel (csrc/predict_small_tree.hip): every p[f] carries `tree`, a ffgp_ktree of
   2-4 leaves in the FFGP_TREE_CHAIN / FFGP_TREE_BALANCED shapes with Sum / Product nodes, leaves FFGP_KFUN_SE ... FFGP_KFUN_MATERN52
   (w_dev one broadcast value or D) and FFGP_KFUN_LINEAR (centre at the origin, or given through center_dev) -- what
   ffgp_train_tree_lds_raw trains, described the same way: the leaves on their RAW parameters with links[f] (center_train is not
   read: a centre is used as it stands), or links == NULL for effective parameters and identity links (w_dev then holds D values).
   The limits, ffgp_predict_member, var_add_noise, the status words, the return value, the grid (F, S) and FFGP_PREDICT_SPLIT are
   ffgp_predict_small_batch's; diag_add_dev (required) is the only Sigma extra.  Sigma and K_s are formed entry by entry as the
   one-launch tree trainer forms Sigma (X as given, per leaf sum_k w_ek^2 (x_ik - x_jk)^2 or sum_k w_ek^2 (x_ik - c_k)(x_jk - c_k),
   then the tree node by node), and var_dev[nt] = k(x, x) - colsum(V^2) [+ noise] with k(x, x) the tree on the leaves' self values,
   formed per test point (a linear leaf's depends on it).  A point's results do not depend on S, on its tile or on the other points
   and members of the call, bit for bit; a member whose Sigma is not positive definite stops alone (status, NaN outputs).
   FFGP_ERR_ARG -- before anything is enqueued or written -- for what ffgp_predict_small_batch refuses, tree == NULL or of another
   form, a FFGP_KFUN_RQ leaf, a leaf without w_dev / amp_dev, diag_vec_dev, a missing diag_add_dev.  Synchronous; the handle's
   cached factors stay valid.                                                                                                  */
int ffgp_predict_small_tree_batch(ffgp_handle* h, int F, const ffgp_problem* p, const ffgp_tree_links* links, const ffgp_predict_member* m,
                                  int* status);

/* ---- multi-GPU: the joint likelihood of sharded blocks --------------------------------------------------- */
/* buf_dev[0..count) <- element-wise SUM over the ranks of `comm` (in place, fp64), enqueued on the handle's stream: the ONE
   collective of the per-fidelity sharding -- the F-vector of per-block values, `loss += cigp_list[f].compute_loss(...)`
   in MFGP_ver2023May/ResGP.py:235,245 (the 2024 trainers' per-fidelity loop, FidelityFusion_Models/CIGAR.py:99-134).
   `comm` is the caller's ncclComm_t (RCCL); the library resolves ncclAllReduce from librccl.so.1 at the first call
   (dlopen: libffgp.so has no link-time dependency on RCCL, and a process that already loaded RCCL -- torch -- shares it).
   Returns FFGP_ERR_ARG for bad arguments, FFGP_ERR_HIP if RCCL cannot be loaded or reports an error.              */
int ffgp_allreduce_sum(ffgp_handle* h, void* comm, double* buf_dev, int count);

/* ---- instrumentation ------------------------------------------------------------------------------------ */
/* stage timings (ms) of the last fused call when option "timing" = 1; names are static strings */
int ffgp_last_timings(ffgp_handle* h, float* ms_out, const char** names_out, int max_stages, int* n_stages);
/* accumulated launches / algorithmic flops / device ms of the trailing-update SYRK kernel (the roofline kernel);
   reset = 1 clears the counters after reading.  ms is only accumulated while option "timing" = 2.           */
int ffgp_syrk_stats(ffgp_handle* h, double* flops, double* ms, long* launches, int reset);
/* peak probe: runs a register-resident v_mfma_f64_16x16x4_f64 loop on every CU, returns measured TFLOP/s */
int ffgp_mfma_f64_peak(ffgp_handle* h, double* tflops_out);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FFGP_H */

// Symmetric eigendecomposition for n <= 128 in ONE workgroup (the N x N input kernel of the HOGP block at GAR's sizes:
// two_fidelity_models/hogp_simple.py:15-19 on 100 low-fidelity points, Experiments/GAR_Aligned/exp_aligned.py:66-99).
//
// ffgp_syev_lds: batched, one workgroup per matrix, one launch.  The two-sided Jacobi of eig.hip keeps A and the accumulated
//   rotations in LDS: two [128][129] fp64 images are 264 KB, the CU has 160 KiB.  This kernel keeps ONE image: one-sided
//   (Hestenes) Jacobi on G = A + s I with s = 1.5 min(Gershgorin radius, ||A||_F) >= 1.5 rho(A), so that G is positive
//   definite with cond(G) <= 5, its singular values are its eigenvalues (no +-lambda mixing) and no column norm is small.
//   Rotating the columns of G from the right until they are mutually orthogonal leaves G V = U Sigma in place; G is symmetric
//   positive definite, so U = V up to rounding and the normalised columns are the eigenvectors -- V is never stored.  The
//   eigenvalues are Rayleigh quotients u^T A u against the untouched input (sigma - s would cancel).  The image is scaled
//   by a power of two so that the radius is in [1, 2) (exact; keeps the squares in range for any finite input), and the norms
//   are taken of the scaled image.  A NaN or Inf anywhere in the lower triangle gives NaN outputs and info = n.
//   Pairing: the round-robin tournament of eig.hip (a dummy player for odd n); a pair of columns belongs to 16 lanes of one
//   wave, which hold both columns in registers, reduce their dot product by a butterfly (every lane gets the same bits) and
//   write the rotated columns back: the pairs of a step are disjoint, so a step costs one barrier.  A pair rotates while
//   |g_p . g_q| > eps ||g_p|| ||g_q||; a sweep without a rotation ends the iteration, EL_MAX_SWEEPS bounds it.
//   A step is a chain of dependent operations between two barriers, so the kernel is built to keep that chain short: the image
//   is padded with zero rows to a multiple of 16 (rotations keep them zero: no bounds checks in the loop; the kernel is
//   instantiated per row count), the 16-lane sums are DPP moves inside a row of lanes, and the angle comes from hardware
//   reciprocal estimates with one Newton step each; the rotation's scale is then corrected to first order (see the loop).
#include "ffgp_internal.h"

#define EL_MAX_N FFGP_SYEV_LDS_MAX_N
#define EL_MAX_SWEEPS 40
#define EL_GROUP 16                      // lanes per column pair (one DPP row)

struct SyevLdsArgs {
  const double* M; int n; int ldm; long sM;
  double* Q; int ldq; long sQ;
  double* evals; long sE;
  int descending;
  int* info;
};

// (tests/test_eig_lds_isa.py restates the next four functions to add up the LDS request and looks for their text: change both)
static inline int el_threads(int n) { return n > 64 ? 1024 : n > 32 ? 512 : 256; }
static inline int el_rows(int n) { return n > 64 ? (n + EL_GROUP - 1) / EL_GROUP : 4; }      // rows of a column per lane: 4 .. 8
static inline int el_ld(int n) { return EL_GROUP * el_rows(n) + 1; }                          // odd: columns start in different banks
// dynamic LDS: the image [n][ld] (column p of G at C + p * ld) and the waves' partial Rayleigh quotients [waves][n]
static inline size_t el_lds_bytes(int n) { return ((size_t)n * el_ld(n) + (size_t)(el_threads(n) / 64) * n) * sizeof(double); }

// sum over the 16 lanes of a DPP row; every lane gets the same bits (each stage adds the same two numbers in both lanes)
template <int CTRL>
__device__ __forceinline__ double el_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double el_sum16(double v) {
  v += el_dpp<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += el_dpp<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += el_dpp<0x141>(v);   // row_half_mirror
  v += el_dpp<0x140>(v);   // row_mirror
  return v;
}

// (1 - c^2 - s^2) / 2 to ~1e-32 for c^2 + s^2 near 1: 1 - c2 and (1 - c2) - s2 are exact differences, the fused products give the
// rounding errors of c2 and s2.  Contraction is off: a product fused into a subtraction here would count its error twice.
__device__ __forceinline__ double el_half_defect(double c, double s) {
#pragma clang fp contract(off)
  const double c2 = c * c, s2 = s * s;
  return 0.5 * ((((1.0 - c2) - s2) - __builtin_fma(c, c, -c2)) - __builtin_fma(s, s, -s2));
}

template <int NR>      // rows per lane: the image has 16 NR rows, rows n.. are zero
__global__ __launch_bounds__(1024) void ffgp_syev_lds_kernel(SyevLdsArgs a) {
  extern __shared__ double el_smem[];
  __shared__ double rabs[EL_MAX_N], rsq[EL_MAX_N], lam[EL_MAX_N], nrm[EL_MAX_N];
  __shared__ int rank_[EL_MAX_N];
  __shared__ int nrot;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int n = a.n;
  constexpr int ld = EL_GROUP * NR + 1;
  double* __restrict__ C = el_smem;
  double* __restrict__ part = el_smem + (size_t)n * ld;
  const double* __restrict__ M = a.M + (size_t)blockIdx.x * a.sM;
  double* __restrict__ Q = a.Q + (size_t)blockIdx.x * a.sQ;
  double* __restrict__ ev = a.evals + (size_t)blockIdx.x * a.sE;

  // the lower triangle, mirrored; zero rows below
  for (int idx = tid; idx < n * (ld - 1 - n); idx += nt) {
    const int j = idx / (ld - 1 - n), i = n + idx - j * (ld - 1 - n);
    C[j * ld + i] = 0.0;
  }
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    if (j <= i) {
      const double v = M[(size_t)i * a.ldm + j];
      C[i * ld + j] = v;
      C[j * ld + i] = v;
    }
  }
  __syncthreads();
  if (tid < n) {
    double sa = 0.0;
    for (int j = 0; j < n; ++j) sa += fabs(C[tid * ld + j]);
    rabs[tid] = sa;
  }
  __syncthreads();
  // Gershgorin's radius.  Every element sits in some row sum, so one NaN or Inf anywhere makes a row sum non-finite; the comparison
  // is written so that a NaN is kept (fmax would drop it).
  double gersh = 0.0;
  bool finite = true;
  for (int i = 0; i < n; ++i) {
    const double r = rabs[i];
    finite = finite && (r < __builtin_inf());      // false for NaN too (and for a row sum that overflows)
    gersh = (r > gersh) ? r : gersh;
  }
  if (!finite || gersh == 0.0) {
    // zero matrix: zeros and the identity.  Inf / NaN anywhere in the lower triangle: NaN out, info = n.
    const double fill = finite ? 0.0 : __builtin_nan("");
    for (int idx = tid; idx < n * n; idx += nt) {
      const int i = idx / n, j = idx - i * n;
      Q[(size_t)i * a.ldq + j] = finite ? (i == j ? 1.0 : 0.0) : fill;
    }
    if (tid < n) ev[tid] = fill;
    if (tid == 0 && a.info) a.info[blockIdx.x] = finite ? 0 : n;
    return;
  }
  // scale by a power of two so that the radius is in [1, 2) (exact), THEN take the Frobenius norm: squares of the unscaled entries
  // could be denormal (entries ~1e-160) and the sum come out short of the true norm, which the shift's bound rests on
  const int sc = -ilogb(gersh);
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    C[i * ld + j] = ldexp(C[i * ld + j], sc);
  }
  __syncthreads();
  if (tid < n) {
    double sq = 0.0;
    for (int j = 0; j < n; ++j) {
      const double v = C[tid * ld + j];
      sq = fma(v, v, sq);
    }
    rsq[tid] = sq;
  }
  __syncthreads();
  double fro2 = 0.0;
  for (int i = 0; i < n; ++i) fro2 += rsq[i];
  const double fro = sqrt(fro2), gs = ldexp(gersh, sc);      // fro >= gs / sqrt(n) > 0 (the radius is one row's 1-norm)
  const double shift = 1.5 * (fro < gs ? fro : gs);           // in [1.5 / sqrt(n), 3): the image's entries are O(1)
  __syncthreads();                                            // (rsq is read above; the diagonal is written below)
  if (tid < n) C[tid * ld + tid] += shift;
  __syncthreads();

  // ---- one-sided Jacobi on the columns of G --------------------------------------------------------------------------------
  const int grp = tid / EL_GROUP, l = tid % EL_GROUP, ngrp = nt / EL_GROUP;
  const int m = n + (n & 1), npair = m >> 1;   // players (one dummy for odd n), pairs per step
  const double tol2 = 2.220446049250313e-16 * 2.220446049250313e-16;
  int rotated = 0;
  for (int sweep = 0; sweep < EL_MAX_SWEEPS; ++sweep) {
    if (tid == 0) nrot = 0;
    // the columns' squared norms, fresh every sweep; a rotation updates its two (they only steer the angle and scale the
    // threshold -- the dot product that decides is recomputed every time)
    for (int k = grp; k < n; k += ngrp) {
      const double* __restrict__ cp = C + k * ld + l;
      double aa = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const double x = cp[EL_GROUP * r];
        aa = fma(x, x, aa);
      }
      aa = el_sum16(aa);
      if (l == 0) nrm[k] = aa;
    }
    __syncthreads();
    int mine = 0;
    for (int step = 0; step < m - 1; ++step) {
      for (int k = grp; k < npair; k += ngrp) {
        int p, q;
        if (k == 0) {
          p = m - 1;
          q = step;
        } else {           // (step + k) mod (m - 1), (step - k) mod (m - 1)
          p = step + k;
          if (p >= m - 1) p -= m - 1;
          q = step - k;
          if (q < 0) q += m - 1;
        }
        if (p >= n || q >= n) continue;          // the dummy player sits out
        double* __restrict__ cp = C + p * ld + l;
        double* __restrict__ cq = C + q * ld + l;
        const double aa = nrm[p], bb = nrm[q];
        double x[NR], y[NR];
        double dd = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          x[r] = cp[EL_GROUP * r];
          y[r] = cq[EL_GROUP * r];
          dd = fma(x[r], y[r], dd);
        }
        dd = el_sum16(dd);
        if (!(dd * dd <= tol2 * aa * bb)) {   // the same bits in the 16 lanes: a uniform decision per pair
          // tan of the angle that zeroes g_p . g_q, the smaller root: t = 2 d / (h + sign(h) sqrt(h^2 + 4 d^2)), h = b - a.  Its
          // accuracy only sets how close to zero the product lands (hardware estimates + one Newton step: ~1e-13).  What must
          // hold to rounding is the rotation's orthogonality: [c -s; s c] is a rotation times sqrt(c^2 + s^2) for ANY c and s, and a
          // scale that differs from 1 is a column scaling of G the iteration never undoes (measured: a scale off by 1 ulp per
          // rotation doubles the reconstruction error).  So c = 1 / sqrt(1 + t^2) comes from an estimate too, the defect
          // rho = 1 - c^2 - s^2 is evaluated exactly (fused products and their errors) and the rotated columns take (1 + rho / 2).
          const double h = bb - aa;
          const double r2 = fma(h, h, 4.0 * dd * dd);
          double y0 = __builtin_amdgcn_rsq(r2);
          y0 = y0 * fma(-0.5 * r2, y0 * y0, 1.5);
          const double den = h + copysign(r2 * y0, h);
          double i0 = __builtin_amdgcn_rcp(den);
          i0 = i0 * fma(-den, i0, 2.0);
          const double t = 2.0 * dd * i0;
          const double w = fma(t, t, 1.0);
          double c = __builtin_amdgcn_rsq(w);
          c = c * fma(-0.5 * w, c * c, 1.5);
          const double s = t * c;
          const double hr = el_half_defect(c, s);
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const double zx = fma(c, x[r], -s * y[r]), zy = fma(s, x[r], c * y[r]);
            cp[EL_GROUP * r] = fma(zx, hr, zx);
            cq[EL_GROUP * r] = fma(zy, hr, zy);
          }
          if (l == 0) {
            nrm[p] = aa - t * dd;
            nrm[q] = bb + t * dd;
            ++mine;
          }
        }
      }
      __syncthreads();
    }
    if (mine) atomicAdd(&nrot, mine);
    __syncthreads();
    rotated = nrot;
    __syncthreads();
    if (rotated == 0) break;   // uniform
  }

  // ---- normalise the columns: U --------------------------------------------------------------------------------------------
  for (int k = grp; k < n; k += ngrp) {
    double* __restrict__ cp = C + k * ld + l;
    double x[NR];
    double aa = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      x[r] = cp[EL_GROUP * r];
      aa = fma(x[r], x[r], aa);
    }
    const double nr = sqrt(el_sum16(aa));
#pragma unroll
    for (int r = 0; r < NR; ++r) cp[EL_GROUP * r] = x[r] / nr;   // (a division: a column that never rotated -- a diagonal input -- comes out as exactly e_k)
  }
  __syncthreads();

  // ---- Rayleigh quotients against the input's lower triangle:  u^T A u = 2 sum_i u_i (sum_{k<i} a_ik u_k + a_ii u_i / 2) --------
  // a wave owns rows w, w + waves, ...; its lanes own columns lane and lane + 64; the row of A is wave-uniform
  {
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nt >> 6, lane = tid & 63;
    const int j0 = lane, j1 = lane + 64;
    const double* __restrict__ u0 = C + (j0 < n ? j0 : 0) * ld;
    const double* __restrict__ u1 = C + (j1 < n ? j1 : 0) * ld;
    double acc0 = 0.0, acc1 = 0.0;
    for (int i = w; i < n; i += nw) {
      const double* __restrict__ row = M + (size_t)i * a.ldm;
      double t0 = 0.0, t1 = 0.0;
#pragma unroll 4
      for (int k = 0; k < i; ++k) {
        const double v = row[k];
        t0 = fma(v, u0[k], t0);
        t1 = fma(v, u1[k], t1);
      }
      const double hd = 0.5 * row[i];
      t0 = fma(hd, u0[i], t0);
      t1 = fma(hd, u1[i], t1);
      acc0 = fma(u0[i], t0, acc0);
      acc1 = fma(u1[i], t1, acc1);
    }
    if (j0 < n) part[w * n + j0] = acc0;
    if (j1 < n) part[w * n + j1] = acc1;
    __syncthreads();
    if (tid < n) {
      double sum = 0.0;
      for (int ww = 0; ww < nw; ++ww) sum += part[ww * n + tid];
      lam[tid] = 2.0 * sum;
    }
  }
  __syncthreads();

  // ---- order (ties by index, as eig.hip) and write ------------------------------------------------------------------------------
  if (tid < n) {
    const double di = lam[tid];
    int r = 0;
    for (int j = 0; j < n; ++j) {
      if (j == tid) continue;
      const double dj = lam[j];
      bool before;   // does j come before tid?
      if (dj != di) before = a.descending ? (dj > di) : (dj < di);
      else before = j < tid;
      r += before ? 1 : 0;
    }
    rank_[tid] = r;
    ev[r] = di;
  }
  __syncthreads();
  for (int idx = tid; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    Q[(size_t)i * a.ldq + rank_[j]] = C[j * ld + i];
  }
  if (tid == 0 && a.info) a.info[blockIdx.x] = rotated;
}

int ffgp_syev_lds_impl(ffgp_handle* h, const double* M, int n, int ldm, int batch, long strideM, double* Q, int ldq, long strideQ,
                       double* evals, long strideE, int descending, int* info) {
  if (!M || !Q || !evals || n < 1 || n > EL_MAX_N || ldm < n || ldq < n) return FFGP_ERR_ARG;
  if (batch <= 0) return FFGP_OK;
  void (*const kern[5])(SyevLdsArgs) = {ffgp_syev_lds_kernel<4>, ffgp_syev_lds_kernel<5>, ffgp_syev_lds_kernel<6>, ffgp_syev_lds_kernel<7>,
                                         ffgp_syev_lds_kernel<8>};
  // (unsynchronised on purpose, as train.hip's: two host threads that both find it false set the same attribute twice, which is
  // harmless; a device index outside the table sets it on every call)
  static bool attr_set[64] = {false};
  if (h->device < 0 || h->device >= 64 || !attr_set[h->device]) {
    for (int r = 4; r <= 8; ++r)      // the largest n of each instantiation
      FFGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern[r - 4]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)el_lds_bytes(EL_GROUP * r)));
    if (h->device >= 0 && h->device < 64) attr_set[h->device] = true;
  }
  SyevLdsArgs a;
  a.M = M; a.n = n; a.ldm = ldm; a.sM = strideM;
  a.Q = Q; a.ldq = ldq; a.sQ = strideQ;
  a.evals = evals; a.sE = strideE;
  a.descending = descending;
  a.info = info;
  hipLaunchKernelGGL(kern[el_rows(n) - 4], dim3(batch), dim3(el_threads(n)), el_lds_bytes(n), h->stream, a);
  if (hipGetLastError() != hipSuccess) return FFGP_ERR_HIP;
  return FFGP_OK;
}

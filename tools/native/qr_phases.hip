// Where the time of the band reduction's panel QR goes (development probe): the library's own kernels, compiled here with 100 MHz clock
// stamps of workgroup 0 / thread 0 (FFGP_QR_STAMPS in csrc/sy2sb.hip), on a random 8160 x 32 panel with the matrix's row stride.
// Prints the time of the leaf QR launch and the phases of sy2sb_top on the same panel.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ifidelityfusion_amd/csrc tools/native/qr_phases.hip \
//         -Lfidelityfusion_amd -lffgp -Wl,-rpath,$PWD/fidelityfusion_amd -o qr_phases && ./qr_phases
#define FFGP_QR_STAMPS 1
// (own names for the two kernels launched here: the library linked below exports the unstamped ones under the original names, and
//  with equal names the loader binds both registrations to one handle -- the library's code object then runs)
#define sy2sb_leaf_qr probe_leaf_qr
#define sy2sb_top probe_top
#include "../../fidelityfusion_amd/csrc/sy2sb.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                       \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      printf("%s: %s\n", #x, hipGetErrorString(e_));                                \
      return 1;                                                                     \
    }                                                                               \
  } while (0)

int main() {
  const int n = 8192, m = 8160, L = (m + QR_ROWS - 1) / QR_ROWS;
  std::vector<double> hA((size_t)m * 32);
  srand(1);
  for (auto& v : hA) v = (double)rand() / RAND_MAX - 0.5;
  double *A, *Rst, *Tst;
  CK(hipMalloc(&A, (size_t)m * n * sizeof(double)));
  CK(hipMalloc(&Rst, (size_t)L * 1024 * sizeof(double)));
  CK(hipMalloc(&Tst, (size_t)L * 1024 * sizeof(double)));
  LeafArgs la;
  la.A = A; la.lda = n; la.m = m; la.Rst = Rst; la.Tst = Tst;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float best = 1e9f;
  for (int rep = 0; rep < 5; ++rep) {
    CK(hipMemcpy2D(A, (size_t)n * sizeof(double), hA.data(), 32 * sizeof(double), 32 * sizeof(double), m, hipMemcpyHostToDevice));
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(sy2sb_leaf_qr, dim3(L), dim3(QR_THREADS), 0, 0, la);
    CK(hipGetLastError());
    CK(hipEventRecord(e1, 0));
    CK(hipDeviceSynchronize());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (ms < best) best = ms;
  }
  printf("sy2sb_leaf_qr (1024 threads): %.1f us (events, best of 5, %d leaves)\n", best * 1e3, L);
  unsigned long long st[64];
  auto us = [&](int a, int b) { return (double)(st[b] - st[a]) * 0.01; };
  // the top kernel of the same panel: QR of the 16 stacked R factors, then the reconstruction algebra (one workgroup)
  double *Vtst, *small, *Tpan, *Yp, *ABp;
  CK(hipMalloc(&Vtst, 512 * 32 * sizeof(double)));
  CK(hipMalloc(&small, 4096 * sizeof(double)));
  CK(hipMalloc(&Tpan, 1024 * sizeof(double)));
  CK(hipMalloc(&Yp, (size_t)32 * 32 * sizeof(double)));
  CK(hipMalloc(&ABp, (size_t)32 * SB_LDB * sizeof(double)));
  CK(hipMemcpy2D(A, (size_t)n * sizeof(double), hA.data(), 32 * sizeof(double), 32 * sizeof(double), m, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe_leaf_qr, dim3(L), dim3(QR_THREADS), 0, 0, la);
  TopArgs ta;
  ta.A = A; ta.lda = n; ta.m = m; ta.L = L; ta.Rst = Rst; ta.Tst = Tst; ta.Vtst = Vtst; ta.small = small;
  ta.Vmid0 = Rst; ta.Tmid0 = Tst; ta.three = 0; ta.Tpan = Tpan; ta.Y = Yp; ta.ldy = 32; ta.AB = ABp; ta.use_tree = 1;
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0, 0));
  hipLaunchKernelGGL(probe_top, dim3(1), dim3(QR_THREADS), 0, 0, ta);
  CK(hipGetLastError());
  CK(hipEventRecord(e1, 0));
  CK(hipDeviceSynchronize());
  float tms;
  CK(hipEventElapsedTime(&tms, e0, e1));
  CK(hipMemcpyFromSymbol(st, HIP_SYMBOL(ffgp_qr_stamp), sizeof(st)));
  printf("sy2sb_top: %.1f us (events).  load %.2f  QR of the R stack %.2f  V / Xt / Q0 %.2f  X0, W, top block of Q1 %.2f  modified LU %.2f  "
         "U, T, U^-1 %.2f  stores %.2f us\n", tms * 1e3, us(30, 31), us(31, 32), us(32, 33), us(33, 34), us(34, 35), us(35, 36), us(36, 37));
  return 0;
}

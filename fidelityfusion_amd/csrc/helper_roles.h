// HELPER_ROLES: which waves of a 512-thread diagonal-block workgroup help wave 0 in stage [A], from the eight waves' SIMD ids.
// Plain C++ apart from one builtin, so that tests/helper_roles_host.cpp expands the very same text on the CPU for every SIMD table.
#pragma once

// wave-uniform value -> scalar register on the device; the value itself on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define FFGP_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define FFGP_UNIFORM(x) (x)
#endif

// The helper waves of stage [A]: the waves that do not share wave 0's SIMD (fp64 MFMAs and the pivot loop's DP-ALU work share a pipe),
// six with two waves per SIMD.  simd[w] = the SIMD of wave w (wave_simd() of diag_block.h), published behind a barrier.  Declares hidx
// (this wave's index among the helpers, -1 for the others) and nh (their number).  The stage loops need nh >= 4 (the inverse's row
// blocks take two columns per helper and have up to seven): a placement that leaves fewer makes all seven other waves helpers.
// Placement is observed behaviour, not a contract, so the hand-out is tested for EVERY table: tests/test_helper_roles_host.py walks all
// 4^8 on the CPU, tests/test_gpu_helper_roles.py runs the kernels under forced tables (the -DFFGP_TEST_ROLES build, libffgp_roles.so).
// (A macro: as an inlined function the same code compiled to a different instruction order, in wave 0's pivot loop of
// ffgp_small_mfma_kernel among other places.)
#define HELPER_ROLES(simd, wave, hidx, nh)          \
  int hidx = -1, nh = 0;                            \
  {                                                 \
    const int s0_ = (simd)[0];                      \
    for (int w_ = 1; w_ < 8; ++w_) {                \
      const bool is_h_ = (simd)[w_] != s0_;         \
      if (is_h_ && w_ == (wave)) hidx = nh;         \
      nh += is_h_ ? 1 : 0;                          \
    }                                               \
    if (nh < 4) {                                   \
      nh = 7;                                       \
      hidx = (wave) - 1;                            \
    }                                               \
    hidx = FFGP_UNIFORM(hidx);                      \
    nh = FFGP_UNIFORM(nh);                          \
  }

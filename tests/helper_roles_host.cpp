// The helper-wave hand-out of the diagonal-block kernels, for every placement the hardware could report: HELPER_ROLES
// (fidelityfusion_amd/csrc/helper_roles.h -- the kernels' own text, expanded here on the CPU) under all 4^8 tables wave -> SIMD, for
// every wave, and what the stage loops make of the roles.  tests/test_helper_roles_host.py builds and runs it (also under
// -fsanitize=address,undefined); build: c++ -std=c++17 -I fidelityfusion_amd/csrc tests/helper_roles_host.cpp
//
// The stride loops themselves live inside kernels, so their index sets are RESTATED here:
//   trailing-update blocks  for (t = 1 + hidx; t < m (m + 1) / 2; t += nh), m = nst - jj
//       potrf.hip `for (int t = 1 + hidx; t < m * (m + 1) / 2; t += nh)` in ffgp_potrf_diag128_v4's stage [A];
//       train_tile.h, the same line of TR_FACTOR_STAGES
//   inverse columns         j = hidx + q2 * nh, q2 = 0, 1, used while j < s (s <= 7: a row block of the inverse has up to seven columns)
//       potrf.hip `const int j = hidx + q2 * nh;` in stage [A], in the last stage's Tl terms, behind the barrier (the store) and in the
//       last row block after the stage loop; train_tile.h, the two lines of TR_FACTOR_STAGES that read the same
#include <cstdio>
#include <cstdlib>

#include "helper_roles.h"

static void roles_of(const int* simd, int wave, int* hidx_out, int* nh_out) {
  HELPER_ROLES(simd, wave, hidx, nh);
  *hidx_out = hidx;
  *nh_out = nh;
}

#define REQUIRE(cond, ...)                                                                               \
  do {                                                                                                   \
    if (!(cond)) {                                                                                       \
      std::printf("helper_roles_host: table %d %d %d %d %d %d %d %d: ", simd[0], simd[1], simd[2], simd[3], simd[4], simd[5], simd[6], \
                  simd[7]);                                                                              \
      std::printf(__VA_ARGS__);                                                                          \
      std::printf("\n");                                                                                 \
      return 1;                                                                                          \
    }                                                                                                    \
  } while (0)

int main() {
  long by_nh[8] = {0, 0, 0, 0, 0, 0, 0, 0}, fallback = 0;
  for (int table = 0; table < 65536; ++table) {
    int simd[8], hidx[8], nh = 0;
    for (int w = 0; w < 8; ++w) simd[w] = (table >> (2 * w)) & 3;
    for (int w = 0; w < 8; ++w) {
      int nh_w;
      roles_of(simd, w, &hidx[w], &nh_w);
      REQUIRE(w == 0 || nh_w == nh, "wave %d sees nh = %d, wave 0 sees %d", w, nh_w, nh);
      nh = nh_w;
    }
    REQUIRE(nh >= 4 && nh <= 7, "nh = %d", nh);
    REQUIRE(hidx[0] == -1, "wave 0 has hidx = %d", hidx[0]);
    // the helpers' indices are exactly 0 .. nh - 1, each once
    int owner[7] = {0, 0, 0, 0, 0, 0, 0}, natural = 0;
    for (int w = 1; w < 8; ++w) {
      REQUIRE(hidx[w] >= -1 && hidx[w] < nh, "wave %d has hidx = %d with nh = %d", w, hidx[w], nh);
      if (hidx[w] >= 0) owner[hidx[w]] += 1;
      natural += simd[w] != simd[0] ? 1 : 0;
    }
    for (int k = 0; k < nh; ++k) REQUIRE(owner[k] == 1, "helper index %d is held by %d waves (nh = %d)", k, owner[k], nh);
    // a helper is a wave off wave 0's SIMD -- unless fewer than four are, then every other wave is one
    for (int w = 1; w < 8; ++w) {
      const bool want = natural >= 4 ? simd[w] != simd[0] : true;
      REQUIRE((hidx[w] >= 0) == want, "wave %d: helper = %d, expected %d", w, hidx[w] >= 0, want);
    }
    REQUIRE(nh == (natural >= 4 ? natural : 7), "nh = %d with %d waves off wave 0's SIMD", nh, natural);
    // trailing-update blocks: the helpers' stride loops partition 1 .. m (m + 1) / 2 - 1 for every number m of remaining block rows
    for (int m = 1; m <= 8; ++m) {
      const int nblk = m * (m + 1) / 2;
      int hits[36];
      for (int t = 0; t < 36; ++t) hits[t] = 0;
      for (int w = 1; w < 8; ++w)
        if (hidx[w] >= 0)
          for (int t = 1 + hidx[w]; t < nblk; t += nh) hits[t] += 1;
      REQUIRE(hits[0] == 0, "block 0 (wave 0's diagonal block) is updated by a helper, m = %d", m);
      for (int t = 1; t < nblk; ++t) REQUIRE(hits[t] == 1, "m = %d: block %d is updated %d times (nh = %d)", m, t, hits[t], nh);
    }
    // inverse columns: hidx and hidx + nh over the helpers give 0 .. 6, each once (a column >= 7 is never used: j < s <= 7)
    int cols[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int w = 1; w < 8; ++w)
      if (hidx[w] >= 0)
        for (int q2 = 0; q2 < 2; ++q2) {
          const int j = hidx[w] + q2 * nh;
          if (j < 7) cols[j] += 1;
        }
    for (int j = 0; j < 7; ++j) REQUIRE(cols[j] == 1, "inverse column %d is computed by %d waves (nh = %d)", j, cols[j], nh);
    by_nh[nh] += 1;
    fallback += natural < 4 ? 1 : 0;
  }
  std::printf("helper_roles_host: 65536 tables clean (nh = 4: %ld, 5: %ld, 6: %ld, 7: %ld, of which fallback: %ld)\n", by_nh[4], by_nh[5],
              by_nh[6], by_nh[7], fallback);
  return 0;
}

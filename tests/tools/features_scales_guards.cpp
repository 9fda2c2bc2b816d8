// The host side of tl_eigen_features_scales (csrc/tl_features.hip) and tl_leafwood_seed_scales (csrc/tl_leafwood.hip) under the
// sanitizers, on a CPU build and without a GPU: the argument checks of the two entry points of DESIGN §26.  Every call here ends
// before a launch (TL_ERR_ARG, or TL_OK for nothing to do).
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tests/tools/features_scales_guards.cpp \
//         treelearn_amd/csrc/tl_features.hip treelearn_amd/csrc/tl_leafwood.hip -o features_scales_guards && ./features_scales_guards
#include <cstdio>
#include <cstdlib>
#include <limits>
#include "../../include/treelearn_hip.h"

static int failures = 0;
#define EXPECT(call, want)                                                    \
  do {                                                                        \
    const int got = (call);                                                   \
    if (got != (want)) { std::printf("line %d: %s = %d, expected %d\n", __LINE__, #call, got, (want)); ++failures; } \
  } while (0)

int main() {
  alignas(64) static double buf[64];
  void* p = buf;
  void* odd8 = reinterpret_cast<char*>(buf) + 8;
  void* odd4 = reinterpret_cast<char*>(buf) + 4;
  void* odd2 = reinterpret_cast<char*>(buf) + 2;
  const int64_t ext[2] = {3, 4};
  const int32_t cols[3] = {5, 4, 10};
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  auto f = [&](void* a) { return static_cast<float*>(a); };
  auto d = [&](void* a) { return static_cast<double*>(a); };
  auto l = [&](void* a) { return static_cast<int64_t*>(a); };
  auto b = [&](void* a) { return static_cast<uint8_t*>(a); };

  // ---- tl_eigen_features_scales: there is no "nothing to do" (n and n_pieces must be >= 1), so every call below must be refused
  const double r2[2] = {0.2, 0.4};
  EXPECT(tl_eigen_features_scales(nullptr, l(p), 10, r2, 2, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), nullptr, 10, r2, 2, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, nullptr, 2, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, nullptr, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, nullptr, 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 1, nullptr, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 1, cols, 3, nullptr, nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 0, r2, 2, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);            // n
  EXPECT(tl_eigen_features_scales(d(p), l(p), -1, r2, 2, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 0, cols, 3, f(p), nullptr), TL_ERR_ARG);           // n_pieces
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 11, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), (int64_t)1 << 40, r2, 2, ext, l(p), (int64_t)1 << 31, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 0, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);           // S
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, -1, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, TL_FEAT_MAX_SCALES + 1, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 1, cols, 0, f(p), nullptr), TL_ERR_ARG);           // F
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 1, cols, TL_FEAT_COUNT + 1, f(p), nullptr), TL_ERR_ARG);
  const int32_t id_high[3] = {0, TL_FEAT_COUNT, 1}, id_neg[3] = {0, -1, 1};
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 1, id_high, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext, l(p), 1, id_neg, 3, f(p), nullptr), TL_ERR_ARG);
  const int64_t ext_neg[2] = {-1, 4}, ext_big[2] = {3, (int64_t)1 << 21};
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext_neg, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r2, 2, ext_big, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  // the radii: exactly S of them are read (each array below is exactly as long as its S: a read past it is the sanitizer's to find)
  const double one_zero[1] = {0.0}, one_neg[1] = {-0.2}, one_nan[1] = {nan}, one_inf[1] = {inf};
  for (const double* r : {one_zero, one_neg, one_nan, one_inf})
    EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r, 1, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  const double equal2[2] = {0.2, 0.2}, desc2[2] = {0.4, 0.2}, nan2[2] = {0.2, nan}, nan2a[2] = {nan, 0.2}, inf2[2] = {0.2, inf};
  for (const double* r : {equal2, desc2, nan2, nan2a, inf2})
    EXPECT(tl_eigen_features_scales(d(p), l(p), 10, r, 2, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  const double mid3[3] = {0.2, 0.4, 0.3}, last4[4] = {0.1, 0.2, 0.3, 0.3}, first4[4] = {0.0, 0.2, 0.3, 0.4};
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, mid3, 3, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, last4, 4, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, first4, 4, ext, l(p), 1, cols, 3, f(p), nullptr), TL_ERR_ARG);
  // good radii of every length, refused for another reason (an id out of range, checked after them): the radii are read to their end and no further
  const double g1[1] = {0.3}, g3[3] = {0.1, 0.2, 0.3}, g4[4] = {0.1, 0.2, 0.3, 0.4};
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, g1, 1, ext, l(p), 1, id_high, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, g3, 3, ext, l(p), 1, id_high, 3, f(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_eigen_features_scales(d(p), l(p), 10, g4, 4, ext, l(p), 1, id_high, 3, f(p), nullptr), TL_ERR_ARG);

  // ---- tl_leafwood_seed_scales
  const tl_leafwood_params good{0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1};
  for (int S = 1; S <= TL_FEAT_MAX_SCALES; ++S)
    for (int k = 1; k <= S; ++k) EXPECT(tl_leafwood_seed_scales(f(p), 0, S, &good, k, b(p), nullptr), TL_OK);        // nothing to do
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 2, &good, 1, b(odd2), nullptr), TL_OK);
  EXPECT(tl_leafwood_seed_scales(nullptr, 0, 2, &good, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 2, &good, 1, nullptr, nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 2, nullptr, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(odd8), 0, 2, &good, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(odd4), 0, 2, &good, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), -1, 2, &good, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 0, &good, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, -1, &good, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, TL_FEAT_MAX_SCALES + 1, &good, 1, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 2, &good, 0, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 2, &good, 3, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 1, &good, 2, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed_scales(f(p), 0, 4, &good, -1, b(p), nullptr), TL_ERR_ARG);
  const tl_leafwood_params bad[] = {
      {0.0, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1}, {nan, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1}, {0.2, 1.1, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1},
      {0.2, 0.6, nan, 0.2, 0.1, 5, 2, 50, 1, 20, 1}, {0.2, 0.6, 0.3, -0.1, 0.1, 5, 2, 50, 1, 20, 1}, {0.2, 0.6, 0.3, 0.2, inf, 5, 2, 50, 1, 20, 1},
      {0.2, 0.6, 0.3, 0.2, 0.1, 2, 2, 50, 1, 20, 1}, {0.2, 0.6, 0.3, 0.2, 0.1, 5, 9, 50, 1, 20, 1},  {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 0, 1, 20, 1},
      {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 3, 20, 1}, {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 0, 1},   {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 2}};
  for (const tl_leafwood_params& w : bad) EXPECT(tl_leafwood_seed_scales(f(p), 0, 2, &w, 1, b(p), nullptr), TL_ERR_ARG);
  std::printf(failures ? "%d failures\n" : "features_scales_guards: all guards hold\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

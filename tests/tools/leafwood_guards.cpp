// The host side of csrc/tl_leafwood.hip under the sanitizers, on a CPU build and without a GPU: the parameter checks and launch guards
// of the two tl_leafwood_* entry points.  Every call here ends before a launch (TL_ERR_ARG, or TL_OK for nothing to do).
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tests/tools/leafwood_guards.cpp \
//         treelearn_amd/csrc/tl_leafwood.hip -o leafwood_guards && ./leafwood_guards
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
  void* q = buf + 32;
  void* odd8 = reinterpret_cast<char*>(buf) + 8;
  void* odd4 = reinterpret_cast<char*>(buf) + 4;
  void* odd2 = reinterpret_cast<char*>(buf) + 2;
  const int64_t ext[2] = {3, 4};
  const tl_leafwood_params good{0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1};
  auto f = [&](void* a) { return static_cast<float*>(a); };
  auto d = [&](void* a) { return static_cast<double*>(a); };
  auto l = [&](void* a) { return static_cast<int64_t*>(a); };
  auto i = [&](void* a) { return static_cast<int32_t*>(a); };
  auto b = [&](void* a) { return static_cast<uint8_t*>(a); };

  // nothing to do: TL_OK after the argument checks, no launch
  EXPECT(tl_leafwood_seed(f(p), 0, &good, b(p), nullptr), TL_OK);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_OK);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(p), &good, b(p), nullptr, nullptr), TL_OK);
  EXPECT(tl_leafwood_vote(d(p), l(p), 5, ext, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_OK);
  // nulls, misaligned pointers, sizes
  EXPECT(tl_leafwood_seed(nullptr, 0, &good, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed(f(p), 0, &good, nullptr, nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed(f(p), 0, nullptr, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed(f(p), -1, &good, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed(f(odd8), 0, &good, b(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_seed(f(p), 0, &good, b(odd2), nullptr), TL_OK);
  EXPECT(tl_leafwood_vote(nullptr, l(p), 0, ext, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), nullptr, 0, ext, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, nullptr, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, nullptr, 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, nullptr, &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(p), nullptr, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(p), &good, nullptr, i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(odd4), l(p), 0, ext, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(odd4), 0, ext, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(odd4), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(odd2), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(p), &good, b(p), i(odd2), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(odd4), &good, b(odd2), i(q), nullptr), TL_OK);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(p), &good, b(p), i(p), nullptr), TL_ERR_ARG);          // tag_out == tag
  EXPECT(tl_leafwood_vote(d(p), l(p), -1, ext, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), -1, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 1, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);          // n_pieces > n
  EXPECT(tl_leafwood_vote(d(p), l(p), (int64_t)1 << 40, ext, l(p), (int64_t)1 << 31, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  const int64_t ext_neg[2] = {-1, 4}, ext_big[2] = {3, (int64_t)1 << 21};
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext_neg, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext_big, l(p), 0, i(p), &good, b(p), i(q), nullptr), TL_ERR_ARG);
  // every constraint of the parameter table
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const tl_leafwood_params bad[] = {
      {0.0, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1},  {nan, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1},  {inf, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1},
      {0.2, -0.1, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1}, {0.2, 1.1, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1},  {0.2, nan, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 1},
      {0.2, 0.6, -0.1, 0.2, 0.1, 5, 2, 50, 1, 20, 1}, {0.2, 0.6, 1.1, 0.2, 0.1, 5, 2, 50, 1, 20, 1},  {0.2, 0.6, nan, 0.2, 0.1, 5, 2, 50, 1, 20, 1},
      {0.2, 0.6, 0.3, -0.1, 0.1, 5, 2, 50, 1, 20, 1}, {0.2, 0.6, 0.3, 1.1, 0.1, 5, 2, 50, 1, 20, 1},  {0.2, 0.6, 0.3, nan, 0.1, 5, 2, 50, 1, 20, 1},
      {0.2, 0.6, 0.3, 0.2, 0.0, 5, 2, 50, 1, 20, 1},  {0.2, 0.6, 0.3, 0.2, nan, 5, 2, 50, 1, 20, 1},  {0.2, 0.6, 0.3, 0.2, inf, 5, 2, 50, 1, 20, 1},
      {0.2, 0.6, 0.3, 0.2, 0.1, 2, 2, 50, 1, 20, 1},  {0.2, 0.6, 0.3, 0.2, 0.1, 5, -1, 50, 1, 20, 1}, {0.2, 0.6, 0.3, 0.2, 0.1, 5, 9, 50, 1, 20, 1},
      {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 0, 1, 20, 1},   {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 101, 1, 20, 1}, {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 0, 20, 1},
      {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 3, 20, 1},  {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 0, 1},   {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, 2},
      {0.2, 0.6, 0.3, 0.2, 0.1, 5, 2, 50, 1, 20, -1}};
  for (const tl_leafwood_params& w : bad) {
    EXPECT(tl_leafwood_seed(f(p), 0, &w, b(p), nullptr), TL_ERR_ARG);
    EXPECT(tl_leafwood_vote(d(p), l(p), 0, ext, l(p), 0, i(p), &w, b(p), i(q), nullptr), TL_ERR_ARG);
  }
  std::printf(failures ? "%d failures\n" : "leafwood_guards: all guards hold\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

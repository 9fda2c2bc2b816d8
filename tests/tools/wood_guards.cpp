// The host side of csrc/tl_wood.hip under the sanitizers, on a CPU build and without a GPU: the parameter checks and launch guards of
// the two tl_wood_* entry points.  Every call here ends before a launch (TL_ERR_ARG, or TL_OK for nothing to do).
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tests/tools/wood_guards.cpp \
//         treelearn_amd/csrc/tl_wood.hip -o wood_guards && ./wood_guards
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
  alignas(8) static double buf[64];
  void* p = buf;
  void* odd4 = reinterpret_cast<char*>(buf) + 4;
  void* odd2 = reinterpret_cast<char*>(buf) + 2;
  const tl_wood_params good{0.03, 0.005, 1.0, 1.0, 1.3, 8};
  auto d = [&](void* q) { return static_cast<double*>(q); };
  auto l = [&](void* q) { return static_cast<int64_t*>(q); };
  auto i = [&](void* q) { return static_cast<int32_t*>(q); };

  // nothing to do: TL_OK after the argument checks, no launch
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(p), i(p), i(p), 3, i(p), nullptr), TL_OK);
  EXPECT(tl_wood_row_nodes(l(p), 5, l(p), 5, i(p), i(p), i(p), 0, i(p), nullptr), TL_OK);
  EXPECT(tl_wood_row_nodes(l(p), 5, l(p), 0, i(p), i(p), i(p), 0, i(p), nullptr), TL_OK);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(odd4), i(odd4), i(odd4), 3, i(odd4), nullptr), TL_OK);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_OK);
  EXPECT(tl_wood_fit(d(p), 5, l(p), l(p), d(p), i(p), l(p), 2, 0, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_OK);
  EXPECT(tl_wood_fit(d(p), 5, l(p), l(p), d(p), i(p), l(p), 0, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_OK);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(odd4), l(p), 2, 3, &good, d(p), l(p), d(p), i(odd4), d(p), d(p), nullptr), TL_OK);
  // nulls, misaligned pointers, sizes
  EXPECT(tl_wood_row_nodes(nullptr, 0, l(p), 5, i(p), i(p), i(p), 3, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(p), nullptr, i(p), 3, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(p), i(p), i(p), 3, nullptr, nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(odd4), 0, l(p), 5, i(p), i(p), i(p), 3, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(odd4), 5, i(p), i(p), i(p), 3, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(odd2), i(p), i(p), 3, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(p), i(p), i(p), 3, i(odd2), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), -1, l(p), 5, i(p), i(p), i(p), 3, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), -1, i(p), i(p), i(p), 0, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), (int64_t)1 << 31, i(p), i(p), i(p), 3, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(p), i(p), i(p), 6, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_row_nodes(l(p), 0, l(p), 5, i(p), i(p), i(p), -1, i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(nullptr, 0, l(p), l(p), d(p), i(p), l(p), 2, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, 3, nullptr, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, 3, &good, d(p), l(p), d(p), i(p), d(p), nullptr, nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(odd4), l(p), d(p), i(p), l(p), 2, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(odd4), d(p), i(p), l(p), 2, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(odd2), l(p), 2, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, 3, &good, d(odd4), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, 3, &good, d(p), l(p), d(p), i(odd2), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), -1, l(p), l(p), d(p), i(p), l(p), 2, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), -1, 3, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, -1, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, (int64_t)1 << 31, &good, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  // every constraint of the parameter table
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const tl_wood_params bad[] = {
      {-0.01, 0.005, 1.0, 1.0, 1.3, 8}, {nan, 0.005, 1.0, 1.0, 1.3, 8},  {inf, 0.005, 1.0, 1.0, 1.3, 8},  {0.03, -0.1, 1.0, 1.0, 1.3, 8},
      {0.03, nan, 1.0, 1.0, 1.3, 8},    {0.03, 1.0, 1.0, 1.0, 1.3, 8},   {0.03, 0.005, inf, 1.0, 1.3, 8}, {0.03, 0.005, nan, 1.0, 1.3, 8},
      {0.03, 0.005, 0.001, 1.0, 1.3, 8}, {0.03, 0.005, 1.0, 0.5, 1.3, 8}, {0.03, 0.005, 1.0, nan, 1.3, 8}, {0.03, 0.005, 1.0, inf, 1.3, 8},
      {0.03, 0.005, 1.0, 1.0, -1.0, 8}, {0.03, 0.005, 1.0, 1.0, nan, 8}, {0.03, 0.005, 1.0, 1.0, inf, 8}, {0.03, 0.005, 1.0, 1.0, 1.3, 2}};
  for (const tl_wood_params& b : bad)
    EXPECT(tl_wood_fit(d(p), 0, l(p), l(p), d(p), i(p), l(p), 2, 3, &b, d(p), l(p), d(p), i(p), d(p), d(p), nullptr), TL_ERR_ARG);
  std::printf(failures ? "%d failures\n" : "wood_guards: all guards hold\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

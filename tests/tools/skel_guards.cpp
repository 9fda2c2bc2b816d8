// The host side of csrc/tl_skeleton.hip under the sanitizers, on a CPU build and without a GPU: the parameter checks and launch guards
// of the four tl_skel_* entry points.  Every call here ends before a launch (TL_ERR_ARG, or TL_OK for nothing to do).
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined tests/tools/skel_guards.cpp \
//         treelearn_amd/csrc/tl_skeleton.hip -o skel_guards && ./skel_guards
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
  const tl_skel_params good{0.1, 0.5, 1.0, 1, 10, 5, 3, 1 << 20};
  auto d = [&](void* q) { return static_cast<double*>(q); };
  auto l = [&](void* q) { return static_cast<int64_t*>(q); };
  auto i = [&](void* q) { return static_cast<int32_t*>(q); };

  // nothing to do: TL_OK after the argument checks, no launch
  EXPECT(tl_skel_voxel_keys(d(p), l(p), 0, d(p), 3, &good, l(p), i(p), nullptr), TL_OK);
  EXPECT(tl_skel_voxel_keys(d(p), l(p), 5, d(p), 0, &good, l(p), i(p), nullptr), TL_OK);
  EXPECT(tl_skel_distance(l(p), 0, l(p), 3, &good, i(p), i(p), nullptr), TL_OK);
  EXPECT(tl_skel_distance(l(p), 5, l(p), 0, &good, i(p), i(p), nullptr), TL_OK);
  EXPECT(tl_skel_nodes(l(p), 0, l(p), 3, &good, i(p), i(p), l(p), l(p), nullptr), TL_OK);
  EXPECT(tl_skel_links(l(p), 5, l(p), d(p), 3, &good, i(p), i(p), l(p), l(p), i(p), 0, i(p), l(p), d(p), i(p), i(p), l(p), nullptr), TL_OK);
  // nulls, misaligned pointers, sizes
  EXPECT(tl_skel_voxel_keys(nullptr, l(p), 0, d(p), 3, &good, l(p), i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_voxel_keys(d(p), l(p), 0, d(p), 3, nullptr, l(p), i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_voxel_keys(d(p), l(odd4), 0, d(p), 3, &good, l(p), i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_voxel_keys(d(p), l(p), 0, d(p), 3, &good, l(p), i(odd2), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_voxel_keys(d(p), l(p), 0, d(p), 3, &good, l(p), i(odd4), nullptr), TL_OK);
  EXPECT(tl_skel_voxel_keys(d(p), l(p), -1, d(p), 3, &good, l(p), i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_voxel_keys(d(p), l(p), 0, d(p), (int64_t)1 << 21, &good, l(p), i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_distance(l(p), (int64_t)1 << 31, l(p), 3, &good, i(p), i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_distance(l(p), 0, l(odd4), 3, &good, i(p), i(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_nodes(l(p), 0, l(p), 3, &good, i(p), i(p), l(odd4), l(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_links(l(p), 0, l(p), d(p), 3, &good, i(p), i(p), l(p), l(p), i(p), 1, i(p), l(p), d(p), i(p), i(p), l(p), nullptr), TL_ERR_ARG);
  EXPECT(tl_skel_links(l(p), 0, l(p), d(p), 3, &good, i(p), i(p), l(p), l(p), i(p), 0, i(p), l(p), d(p), i(p), i(p), nullptr, nullptr), TL_ERR_ARG);
  // every constraint of the parameter table
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const tl_skel_params bad[] = {
      {0.0, 0.5, 1.0, 1, 10, 5, 3, 1 << 20},  {nan, 0.5, 1.0, 1, 10, 5, 3, 1 << 20}, {inf, 0.5, 1.0, 1, 10, 5, 3, 1 << 20},
      {0.1, -0.5, 1.0, 1, 10, 5, 3, 1 << 20}, {0.1, 0.5, nan, 1, 10, 5, 3, 1 << 20}, {0.1, 0.5, 1.0, 0, 10, 5, 3, 1 << 20},
      {0.1, 0.5, 1.0, 3, 10, 5, 3, 1 << 20},  {0.1, 0.5, 1.0, 1, -1, 5, 3, 1 << 20}, {0.1, 0.5, 1.0, 1, 2048, 5, 3, 1 << 20},
      {0.1, 0.5, 1.0, 1, 10, 0, 3, 1 << 20},  {0.1, 0.5, 1.0, 1, 10, 5, 0, 1 << 20}, {0.1, 0.5, 1.0, 1, 10, 5, 1000001, 1 << 20},
      {0.1, 0.5, 1.0, 1, 10, 5, 3, 0}};
  for (const tl_skel_params& b : bad) {
    EXPECT(tl_skel_voxel_keys(d(p), l(p), 0, d(p), 3, &b, l(p), i(p), nullptr), TL_ERR_ARG);
    EXPECT(tl_skel_distance(l(p), 0, l(p), 3, &b, i(p), i(p), nullptr), TL_ERR_ARG);
    EXPECT(tl_skel_nodes(l(p), 0, l(p), 3, &b, i(p), i(p), l(p), l(p), nullptr), TL_ERR_ARG);
    EXPECT(tl_skel_links(l(p), 0, l(p), d(p), 3, &b, i(p), i(p), l(p), l(p), i(p), 0, i(p), l(p), d(p), i(p), i(p), l(p), nullptr), TL_ERR_ARG);
  }
  std::printf(failures ? "%d failures\n" : "skel_guards: all guards hold\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

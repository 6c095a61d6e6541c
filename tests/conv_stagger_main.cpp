// Stand-alone driver of the staggered-start planner of csrc/xai_conv_walk.h for tests/test_cpu_conv_wide.py: nothing of HIP in it, so
// the host compiler builds it alone, also with -fsanitize=address,undefined.
//   conv_stagger plan  K depth tile axis stagger stride  [...]   per case: "refused", or "ok blocks per_iter tile axis mask shift"
//   conv_stagger chain K depth tile axis stagger stride at       the K-blocks of the output at `at` along the axis, in chain order
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "xai_conv_walk.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "plan")) {
    if ((argc - 2) % 6 != 0) return 2;
    for (int i = 2; i + 5 < argc; i += 6) {
      int a[6];
      for (int j = 0; j < 6; ++j) a[j] = std::atoi(argv[i + j]);
      XaiStagger st;
      std::memset(&st, 0x5a, sizeof st);
      if (!xai_stagger_plan(a[0], a[1], a[2], a[3], a[4], a[5], &st)) {
        const unsigned char* raw = reinterpret_cast<const unsigned char*>(&st);
        for (size_t b = 0; b < sizeof st; ++b)
          if (raw[b] != 0x5a) return 3;               // a refused plan leaves *st untouched
        std::printf("refused\n");
        continue;
      }
      std::printf("ok %d %d %d %d %d %d\n", st.blocks, st.per_iter, st.tile, st.axis, st.mask, st.shift);
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "chain")) {
    if (argc != 9) return 2;
    int a[7];
    for (int j = 0; j < 7; ++j) a[j] = std::atoi(argv[2 + j]);
    XaiStagger st;
    if (!xai_stagger_plan(a[0], a[1], a[2], a[3], a[4], a[5], &st)) return 3;
    const int first = xai_stagger_first(st, a[6]);
    for (int t = 0; t < st.blocks; ++t) std::printf("%d ", xai_stagger_block(st, first, t));
    std::printf("\n");
    return 0;
  }
  return 2;
}

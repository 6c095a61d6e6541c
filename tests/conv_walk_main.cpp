// Stand-alone driver of csrc/xai_conv_walk.h for tests/test_cpu_conv_walk.py: the header has nothing of HIP in it, so the host
// compiler builds it alone, also with -fsanitize=address,undefined.
//   conv_walk plan  K S membership grouping order from_zero  [...]   per case: "ok S grouping from_zero" or "refused", then for an
//                                                                    accepted one a line per partial sum, in adding order:
//                                                                    "first step count : block block ..."
//   conv_walk group                                                  per grouping a line of k(m, q) for m, q = 0..3 in MFMA order,
//                                                                    and a line of row(k) for k = 0..15
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
      XaiWalk w;
      std::memset(&w, 0x5a, sizeof w);
      if (!xai_walk_plan(a[0], a[1], a[2], a[3], a[4], a[5], &w)) {
        const unsigned char* raw = reinterpret_cast<const unsigned char*>(&w);
        for (size_t b = 0; b < sizeof w; ++b)
          if (raw[b] != 0x5a) return 3;               // a refused plan leaves *w untouched
        std::printf("refused\n");
        continue;
      }
      std::printf("ok %d %d %d\n", w.splits, w.grouping, w.from_zero);
      for (int p = 0; p < w.splits; ++p) {
        std::printf("%d %d %d :", w.part[p].first, w.part[p].step, w.part[p].count);
        for (int t = 0; t < w.part[p].count; ++t) std::printf(" %d", xai_walk_block(w, p, t));
        std::printf("\n");
      }
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "group")) {
    for (int g = 0; g < 2; ++g) {
      for (int m = 0; m < 4; ++m)
        for (int q = 0; q < 4; ++q) std::printf("%d ", xai_walk_k(g, m, q));
      std::printf("\n");
      for (int k = 0; k < kWalkBlock; ++k) std::printf("%d ", xai_walk_row(g, k));
      std::printf("\n");
    }
    return 0;
  }
  return 2;
}

// Asks csrc/xai_bn_index.h on the host, built by tests/test_cpu_bn_index.py with the host compiler alone (the header needs
// nothing of HIP):
//   lanes (N C HW first count)...  ->  for every lane t in [first, first + count) of the [N][C][HW] tensor one line
//                                      "t  c0 c1 c2 c3  d0 d1 d2 d3": the channels of its flat elements 4t .. 4t+3, c by
//                                      stepping from the lane's first element, d by the two-channel split the kernels use
//                                      where HW >= 4 (-1 four times below that)
//   path (n HW low_bits)...        ->  one line each: 0 scalar, 1 vector, 2 flat vector
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xai_bn_index.h"

static int lanes(int argc, char** argv) {
  if (argc < 5 || argc % 5 != 0) return 2;
  for (int a = 0; a + 5 <= argc; a += 5) {
    const int N = atoi(argv[a]), C = atoi(argv[a + 1]), HW = atoi(argv[a + 2]);
    const long long first = atoll(argv[a + 3]), count = atoll(argv[a + 4]);
    const int64_t n = static_cast<int64_t>(N) * C * HW;
    for (long long t = first; t < first + count; ++t) {
      const XaiBnLane s0 = xai_bn_lane_first(4 * t, n, HW, C);
      XaiBnLane s = s0;
      int c[4], d[4];
      for (int k = 0; k < 4; ++k) {
        c[k] = s.c;
        s = xai_bn_lane_step(s, HW, C);
        d[k] = HW >= 4 ? (k < xai_bn_lane_split(s0, HW) ? s0.c : xai_bn_next_channel(s0.c, C)) : -1;
      }
      printf("%lld %d %d %d %d %d %d %d %d\n", t, c[0], c[1], c[2], c[3], d[0], d[1], d[2], d[3]);
    }
  }
  return 0;
}

static int path(int argc, char** argv) {
  if (argc < 3 || argc % 3 != 0) return 2;
  for (int a = 0; a + 3 <= argc; a += 3)
    printf("%d\n", static_cast<int>(xai_bn_path(atoll(argv[a]), atoi(argv[a + 1]), static_cast<uintptr_t>(strtoull(argv[a + 2], nullptr, 0)))));
  return 0;
}

int main(int argc, char** argv) {
  int rc = 2;
  if (argc >= 2 && strcmp(argv[1], "lanes") == 0) rc = lanes(argc - 2, argv + 2);
  if (argc >= 2 && strcmp(argv[1], "path") == 0) rc = path(argc - 2, argv + 2);
  if (rc == 2) fprintf(stderr, "usage: %s lanes (N C HW first count)... | path (n HW low_bits)...\n", argv[0]);
  return rc;
}

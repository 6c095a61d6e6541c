// Asks the index helpers that csrc/xai_bn_index.h holds for bnrelu_compact_kernels.hip on the host, built by
// tests/test_cpu_bn_compact_index.py with the host compiler alone (the header needs nothing of HIP):
//   images (N C HW first count)...  ->  for every lane t in [first, first + count) of the [N][C][HW] tensor one line
//                                       "t  m0 m1 m2 m3  x0 x1 x2 x3": the image of its flat elements 4t .. 4t+3 by stepping from
//                                       the lane's first element, and their indices in the channel-major [C][N][HW] twin
//   strided (N C H W s)...          ->  one line "Ho Wo" and then, for every compact output in [C][N][Ho][Wo] order, the flat index
//                                       of the side[N][C][H][W] element it reads
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xai_bn_index.h"

static int images(int argc, char** argv) {
  if (argc < 5 || argc % 5 != 0) return 2;
  for (int a = 0; a + 5 <= argc; a += 5) {
    const int N = atoi(argv[a]), C = atoi(argv[a + 1]), HW = atoi(argv[a + 2]);
    const long long first = atoll(argv[a + 3]), count = atoll(argv[a + 4]);
    const int64_t n = static_cast<int64_t>(N) * C * HW;
    for (long long t = first; t < first + count; ++t) {
      XaiBnLane s = xai_bn_lane_first(4 * t, n, HW, C);
      int image = xai_bn_image_first(4 * t, n, HW, C);
      int m[4];
      long long x[4];
      for (int k = 0; k < 4; ++k) {
        m[k] = image;
        x[k] = xai_bn_cnhw_index(image, s.c, s.r, N, HW);
        s = xai_bn_lane_step(s, HW, C);
        image = xai_bn_image_step(image, s);
      }
      printf("%lld %d %d %d %d %lld %lld %lld %lld\n", t, m[0], m[1], m[2], m[3], x[0], x[1], x[2], x[3]);
    }
  }
  return 0;
}

static int strided(int argc, char** argv) {
  if (argc < 5 || argc % 5 != 0) return 2;
  for (int a = 0; a + 5 <= argc; a += 5) {
    const int N = atoi(argv[a]), C = atoi(argv[a + 1]), H = atoi(argv[a + 2]), W = atoi(argv[a + 3]), s = atoi(argv[a + 4]);
    const int Ho = xai_bn_strided_extent(H, s), Wo = xai_bn_strided_extent(W, s);
    printf("%d %d\n", Ho, Wo);
    for (int c = 0; c < C; ++c)
      for (int n = 0; n < N; ++n)
        for (int ho = 0; ho < Ho; ++ho)
          for (int wo = 0; wo < Wo; ++wo) printf("%lld\n", static_cast<long long>(xai_bn_strided_index(n, c, ho, wo, C, H, W, s)));
  }
  return 0;
}

int main(int argc, char** argv) {
  int rc = 2;
  if (argc >= 2 && strcmp(argv[1], "images") == 0) rc = images(argc - 2, argv + 2);
  if (argc >= 2 && strcmp(argv[1], "strided") == 0) rc = strided(argc - 2, argv + 2);
  if (rc == 2) fprintf(stderr, "usage: %s images (N C HW first count)... | strided (N C H W s)...\n", argv[0]);
  return rc;
}

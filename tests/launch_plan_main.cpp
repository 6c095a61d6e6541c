// Prints csrc/xai_launch_plan.h's plan for the cases on the command line, eight numbers each:
//   row_len block vec n C images threshold split  ->  one line "tiles chunks zdim per ok hbm"
// Built by tests/test_cpu_launch_plan.py with the host compiler alone: the header needs nothing of HIP.
#include <stdio.h>
#include <stdlib.h>

#include "xai_launch_plan.h"

int main(int argc, char** argv) {
  if (argc < 9 || (argc - 1) % 8 != 0) {
    fprintf(stderr, "usage: %s (row_len block vec n C images threshold split)...\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 8 <= argc; i += 8) {
    const long long a[8] = {atoll(argv[i]),     atoll(argv[i + 1]), atoll(argv[i + 2]), atoll(argv[i + 3]),
                            atoll(argv[i + 4]), atoll(argv[i + 5]), atoll(argv[i + 6]), atoll(argv[i + 7])};
    const XaiRowPlan p = xai_row_chunk_plan(a[0], static_cast<int>(a[1]), a[2] != 0, static_cast<int>(a[3]), static_cast<int>(a[4]), a[5],
                                            a[6], a[7] != 0);
    printf("%lld %lld %d %d %d %d\n", static_cast<long long>(p.tiles), static_cast<long long>(p.chunks), p.zdim, p.per, p.ok ? 1 : 0,
           p.hbm ? 1 : 0);
  }
  return 0;
}

// Where hbx::pass_launch_small (csrc/hbx_internal.hpp) turns: for every lane-group size R, plane count P
// and job kind (pair = the plane-cached step's one pair per job), the smallest n_jobs of a launch that
// runs the walking forms of the first pass and of k_col2, or "never".  One line per combination:
//   R P pair first_walking_n_jobs
// The sibling of the pass_call_check_*.hip programs; built by tests/test_launch_size_host.py, which
// compares the table with tests/_launch_size.py -- the rule the GPU tests of the two forms
// (tests/test_gpu_launch_size.py) choose their job counts by.  Needs no GPU and no library.
#include <stdio.h>

#include "hbx_internal.hpp"

int main() {
  const int kMaxJobs = 1 << 16;   // far past every crossing (the largest is 256 jobs)
  for (int R : {32, 16, 8})
    for (int P : {2, 4, 8, 12, 24})
      for (int pair : {0, 1}) {
        int first = 0;
        for (int n = 1; n <= kMaxJobs && !first; ++n)
          if (!hbx::pass_launch_small(R, P, n, pair != 0)) first = n;
        // the switch is a threshold: small below the crossing, never again at or above it
        for (int n = 1; n <= kMaxJobs; ++n)
          if (hbx::pass_launch_small(R, P, n, pair != 0) != (first == 0 || n < first)) {
            printf("FAIL R %d P %d pair %d: not a threshold at n_jobs %d\n", R, P, pair, n);
            return 1;
          }
        if (first) printf("%d %d %d %d\n", R, P, pair, first);
        else printf("%d %d %d never\n", R, P, pair);
      }
  return 0;
}

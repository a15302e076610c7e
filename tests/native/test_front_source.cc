// The two rules of a front-end launch's source (csrc/host/lsn_front_source.h, header only): lsn_ring_holds and lsn_window_holds.  A program of its own under the
// address and undefined-behaviour sanitizers.  Arguments, all decimal: cases "r ring_samples window" and "w in_base n_in lo hi"; one line per case - the verdict of
// a ring, or "verdict need_lo len" of a window.  tests/test_front_source.py compares against Python integers.
#include "../../ltesniffer_amd/csrc/host/lsn_front_source.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
  int i = 1;
  while (i < argc) {
    if (argv[i][0] == 'r' && i + 2 < argc) {
      printf("%d\n", lsn_ring_holds(strtoull(argv[i + 1], nullptr, 10), strtoull(argv[i + 2], nullptr, 10)) ? 1 : 0);
      i += 3;
    } else if (argv[i][0] == 'w' && i + 4 < argc) {
      const LsnWindowNeed n = lsn_window_holds(strtoull(argv[i + 1], nullptr, 10), strtoull(argv[i + 2], nullptr, 10), strtoll(argv[i + 3], nullptr, 10), strtoll(argv[i + 4], nullptr, 10));
      printf("%d %lld %llu\n", n.ok ? 1 : 0, (long long)n.lo, (unsigned long long)n.len);
      i += 5;
    } else {
      return 2;
    }
  }
  return 0;
}

// chan_mid_span (csrc/host/lsn_chanfilt.h): the span of its intermediate that stage 2 reads of a resampler piece's input span, and whether it fits.  A program of
// its own under the address and undefined-behaviour sanitizers.  Arguments: groups of four decimal words - lo hi cap L; one line "lo2 hi2 fits" per group.  The
// properties that need no second opinion are checked here (exit status 3, 4); tests/test_chan_mid_span.py compares the values against Python integers.
#include "../../ltesniffer_amd/csrc/host/lsn_chanfilt.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
  if (argc < 5 || (argc - 1) % 4) return 2;
  for (int i = 1; i + 3 < argc; i += 4) {
    const int64_t lo = strtoll(argv[i], nullptr, 10), hi = strtoll(argv[i + 1], nullptr, 10);
    const uint64_t cap = strtoull(argv[i + 2], nullptr, 10);
    lsn::ChanFilter f;
    f.L = (uint32_t)strtoul(argv[i + 3], nullptr, 10);
    int64_t lo2 = -1, hi2 = -1;
    const bool fits = lsn::chan_mid_span(lo, hi, cap, lo2, hi2);
    if (!(0 <= lo2 && lo2 <= hi2)) return 3;
    // what stage 1 reads for [lo2, hi2) lies inside what the launch's source holds for [lo, hi)
    int64_t a = lo, b = hi, a2 = lo2, b2 = hi2;
    f.widen(a, b);
    f.widen(a2, b2);
    if (lo < hi && hi2 > lo2 && !(a <= a2 && b2 <= b)) return 4;
    printf("%lld %lld %d\n", (long long)lo2, (long long)hi2, fits ? 1 : 0);
  }
  return 0;
}

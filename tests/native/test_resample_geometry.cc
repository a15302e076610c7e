// The run geometry of a resampler plan (csrc/host/lsn_resample.h, header only: ResamplePlan::groupOf, runOf, spanAt, and the launch record that carries them).  A
// program of its own under the address and undefined-behaviour sanitizers.  Arguments: groups of four hex words - step_hi step_lo seg_hi seg_lo - and a decimal
// taps; one line "grp run span seg_span" per group: the geometry of a plan whose nominal step is `step`, its own staged span, and the span of a tracked
// segment of that plan at step `seg`.  tests/test_wide_resample_model.py compares against Python integers.
#include "../../ltesniffer_amd/csrc/host/lsn_resample.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
  if (argc < 6 || (argc - 1) % 5) return 2;
  const lsn::ResampleTablePtrs none;
  for (int i = 1; i + 4 < argc; i += 5) {
    uint64_t w[4];
    for (int j = 0; j < 4; j++) w[j] = strtoull(argv[i + j], nullptr, 16);
    lsn::ResamplePlan p;
    p.step = ((lsn::u128)w[0] << 64) | w[1];
    const lsn::u128 seg = ((lsn::u128)w[2] << 64) | w[3];
    p.taps = (uint32_t)strtoul(argv[i + 4], nullptr, 10);
    p.grp = lsn::ResamplePlan::groupOf(p.step);
    p.run = lsn::ResamplePlan::runOf(p.grp);
    p.span = p.spanAt(p.step);
    // both forms of the launch record carry the plan's geometry; the segment's form takes the segment's span and keeps the plan's lanes and run
    const LsnResampleCell k = p.cell(3, 1, none, nullptr, 1);
    const LsnResampleCell s = p.cell(p.position(3), seg, p.spanAt(seg), 7, 5, none, nullptr, 3);
    if (k.grp != p.grp || k.run != p.run || k.span != p.span || s.grp != p.grp || s.run != p.run || s.span != p.spanAt(seg) || s.d_hi != (uint32_t)(seg >> 64)) return 3;
    printf("%u %u %u %u\n", k.grp, k.run, k.span, s.span);
  }
  return 0;
}

// The launch record ResamplePlan::cell forms (csrc/host/lsn_resample.h): position(m0) = start + m0 * step and the step, split into the kernel's words.  A program
// of its own under the address and undefined-behaviour sanitizers.  Arguments: groups of five hex words - start_hi start_lo step_hi step_lo m0; one line
// "base_hi base_lo d_hi d_lo" (hex) per group.  tests/test_resample_cell.py compares against Python integers.
#include "../../ltesniffer_amd/csrc/host/lsn_resample.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
  if (argc < 6 || (argc - 1) % 5) return 2;
  const lsn::ResampleTablePtrs none;
  for (int i = 1; i + 4 < argc; i += 5) {
    uint64_t w[5];
    for (int j = 0; j < 5; j++) w[j] = strtoull(argv[i + j], nullptr, 16);
    lsn::ResamplePlan p;
    p.start = ((lsn::u128)w[0] << 64) | w[1];
    p.step = ((lsn::u128)w[2] << 64) | w[3];
    p.taps = 4; p.span = 16;
    const LsnResampleCell k = p.cell(w[4], 1, none, nullptr, 1);
    if (k.taps != p.taps || k.span != p.span || k.sflen != 1 || k.sf_off != 0 || k.n_out != 1 || k.bank || k.nco || k.rot || k.out || k.w != 0) return 3;
    // the form a tracked segment uses: its own base, step and span, a piece that starts inside its row
    const LsnResampleCell s = p.cell(p.position(w[4]), p.step, 99, 7, 5, none, nullptr, 3);
    if (s.base_hi != k.base_hi || s.base_lo != k.base_lo || s.d_hi != k.d_hi || s.d_lo != k.d_lo || s.taps != p.taps || s.span != 99 || s.sflen != 7 || s.sf_off != 5 || s.n_out != 3) return 4;
    printf("%llx %llx %x %llx\n", (unsigned long long)k.base_hi, (unsigned long long)k.base_lo, k.d_hi, (unsigned long long)k.d_lo);
  }
  return 0;
}

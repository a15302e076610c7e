"""ResamplePlan::cell (csrc/host/lsn_resample.h) - the one place the resampler's host side splits a 64.64 position and step into the kernel's launch words -
against Python integers.  The C++ side is tests/native/test_resample_cell.cc, a program of its own built with -fsanitize=address,undefined."""
import os
import subprocess

from lsn_testlib import ROOT

M64 = (1 << 64) - 1
FRAC_ONES = M64                      # a step whose low word is all ones: m0 * step carries into the high word
CASES = [
    # (start, step, m0)
    (0, 1 << 64, 0),                                                     # m0 = 0, nothing set
    ((7 << 64) | 0x8000000000000001, (1 << 64) | 0x123456789ABCDEF0, 0),  # m0 = 0: base is start itself
    (0, FRAC_ONES, 3),                                                   # 3 * 0xFFFF...F = 2 * 2^64 + 0xFFFF...FD: the low product carries
    (FRAC_ONES, (2 << 64) | FRAC_ONES, 3),                               # ... and the sum with start's fraction carries once more
    ((5 << 64) | 0xC000000000000000, 4 << 64, 1000003),                  # integer part of the step 4 (the largest ratio the plan accepts)
    (0, (4 << 64) | 0xFEDCBA9876543210, 12345678901),
    ((((1 << 62) - 1) << 64) | FRAC_ONES, (1 << 64) | 1, 1),             # start just below 2^62 samples: the sum reaches 2^62
    ((((1 << 62) - 1) << 64) | 0x1, (3 << 64) | 0x8000000000000000, (1 << 40) - 1),
    (123 << 64, 0x5555555555555555, (1 << 40) - 1),                      # m0 just below 2^40, the API's limit: an up-sampling step ...
    ((1 << 64) | FRAC_ONES, (4 << 64) | FRAC_ONES, (1 << 40) - 1),        # ... and the largest step with every low bit set
]


def test_cell_words_equal_python_integers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "_build/test_resample_cell"], stdout=subprocess.DEVNULL)
    args = []
    for start, step, m0 in CASES:
        args += ["%x" % w for w in (start >> 64, start & M64, step >> 64, step & M64, m0)]
    out = subprocess.check_output([os.path.join(ROOT, "tests", "native", "_build", "test_resample_cell")] + args).decode().split("\n")
    rows = [tuple(int(w, 16) for w in line.split()) for line in out if line.strip()]
    assert len(rows) == len(CASES)
    for (start, step, m0), got in zip(CASES, rows):
        P = start + m0 * step
        assert P < (1 << 128) and step >> 64 < (1 << 32)
        assert got == (P >> 64, P & M64, step >> 64, step & M64), (hex(start), hex(step), m0, [hex(g) for g in got])

"""chan_mid_span (csrc/host/lsn_chanfilt.h) - the one place the chain's two stages agree on the span of the intermediate that stage 2 reads of a resampler piece's
input span [lo, hi), and on whether it fits - against Python integers.  The C++ side is tests/native/test_chan_mid_span.cc, a program of its own built with
-fsanitize=address,undefined."""
import os
import random
import subprocess

from lsn_testlib import ROOT

BIG = 1 << 62
CASES = [
    # (lo, hi, cap, L)
    (-95, 30720, 1 << 20, 127),              # lo < 0 < hi: the first block of a replay
    (-95, 30720, 30720, 127),                # ... whose part behind sample 0 is exactly cap samples
    (-95, 30720, 30719, 127),                # ... and one more than cap
    (-4000, -17, 1 << 20, 512),              # hi < 0: the whole piece in front of the recording - the empty span at 0
    (-4000, 0, 0, 512),                      # hi = 0: empty as well, and an empty span fits an intermediate of nothing
    (0, 1, 0, 1),                            # one sample, nothing to hold it
    (0, 30815, 30815, 127),                  # lo = 0, exactly cap
    (0, 30816, 30815, 127),                  # lo = 0, cap + 1
    (7, 7, 0, 3),                            # an empty span behind sample 0 stays where it is
    (123456, 123456 + 65536, 65536, 512),    # exactly cap, away from 0
    (123456, 123456 + 65537, 65536, 512),    # cap + 1
    (BIG - 70000, BIG - 1, 69999, 512),      # near 2^62 (the API's limit on a position): exactly cap
    (BIG - 70000, BIG - 1, 69998, 512),      # ... and cap + 1
    (BIG - 3, BIG + 1024, 1 << 40, 512),     # across 2^62
    (-BIG, BIG, BIG, 512),                   # the widest span the limits allow: its part behind 0 is exactly cap
    (-BIG, BIG, BIG - 1, 512),
    (0, BIG, (1 << 64) - 1, 0),              # the largest cap, no filter
]


def seeded(n, seed):
    """spans about sample 0, about 2^62 and in between, caps about their lengths"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        base = rnd.choice([0, 0, rnd.randrange(1 << 40), BIG - (1 << 20)])
        lo = base + rnd.randrange(-5000, 5000)
        hi = lo + rnd.randrange(0, 1 << rnd.randrange(1, 24))
        want = max(hi, max(lo, 0)) - max(lo, 0)
        out.append((lo, hi, max(0, want + rnd.choice([-1, 0, 0, 1, rnd.randrange(-4000, 4000)])), rnd.randrange(0, 513)))
    return out


def test_mid_span_equals_python_integers():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "_build/test_chan_mid_span"], stdout=subprocess.DEVNULL)
    cases = CASES + seeded(400, 20261)
    args = [str(w) for case in cases for w in case]
    out = subprocess.check_output([os.path.join(ROOT, "tests", "native", "_build", "test_chan_mid_span")] + args).decode().split("\n")
    rows = [tuple(int(w) for w in line.split()) for line in out if line.strip()]
    assert len(rows) == len(cases)
    hit = set()
    for (lo, hi, cap, L), (lo2, hi2, fits) in zip(cases, rows):
        what = (lo, hi, cap, L, lo2, hi2, fits)
        assert 0 <= lo2 <= hi2, what
        if max(lo, 0) < hi:      # [lo, hi) n [0, inf) is not empty: the span is that
            assert (lo2, hi2) == (max(lo, 0), hi), what
            assert lo - L <= lo2 - L and hi2 + L <= hi + L, what   # stage 1's reads for it lie inside the reads of the launch's source for [lo, hi)
        else:                    # empty: no sample, at 0 or where the empty span lies
            assert lo2 == hi2 == max(lo, 0), what
        assert fits == (1 if hi2 - lo2 <= cap else 0), what
        hit.add(("neg" if lo < 0 else "zero" if lo == 0 else "pos", "empty" if hi2 == lo2 else "some", fits, hi2 - lo2 - cap if abs(hi2 - lo2 - cap) <= 1 else None))
    # the cases the span can go wrong at are all in the list
    for need in [("neg", "some", 1, 0), ("neg", "some", 0, 1), ("neg", "empty", 1, 0), ("zero", "some", 1, 0), ("zero", "some", 0, 1), ("pos", "some", 1, 0), ("pos", "some", 0, 1)]:
        assert need in hit, need

"""The two rules every path to a front-end launch checks its source by (csrc/host/lsn_front_source.h), without a GPU: the ring rule - a power of two
of at most 2^32 samples that holds the window - and "the window [in_base, in_base + n_in) holds what outputs that read [lo, hi) need", with the clamped start and
the length it hands the caller.  The C++ side is tests/native/test_front_source.cc, a program of its own built with -fsanitize=address,undefined; this side is the
same rules in Python integers."""
import os
import subprocess

from lsn_testlib import ROOT

RINGS = (0, 1, 2, 3, 2 ** 32, 2 ** 32 + 1, 2 ** 32 * 2)
TOP = 2 ** 62 - 1                    # the largest in_base and n_in the entry points let through


def _run(args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-f", "front_source.mk", "_build/test_front_source"], stdout=subprocess.DEVNULL)
    out = subprocess.check_output([os.path.join(ROOT, "tests", "native", "_build", "test_front_source")] + [str(a) for a in args]).decode()
    return [tuple(int(w) for w in line.split()) for line in out.split("\n") if line.strip()]


def test_ring_rule():
    cases = [(r, w) for r in RINGS for w in sorted({0, 1, r - 1 if r else 0, r, r + 1, 2 ** 32, TOP})]
    got = _run([a for r, w in cases for a in ("r", r, w)])
    assert len(got) == len(cases)
    for (r, w), (ok,) in zip(cases, got):
        assert ok == int(r > 0 and r & (r - 1) == 0 and r <= 2 ** 32 and w <= r), (r, w, ok)
    # what the list above must have met: the two accepted sizes at both ends, a full ring, and each way to fail
    verdict = dict(zip(cases, (g[0] for g in got)))
    assert verdict[(1, 1)] == verdict[(2, 2)] == verdict[(2 ** 32, 2 ** 32)] == verdict[(2 ** 32, 0)] == 1
    assert verdict[(0, 0)] == verdict[(3, 1)] == verdict[(2, 3)] == verdict[(2 ** 32, 2 ** 32 + 1)] == verdict[(2 ** 32 + 1, 1)] == verdict[(2 ** 33, 1)] == 0


def test_window_rule():
    cases = []
    for in_base, n_in in ((0, 0), (0, 1000), (100, 0), (100, 1000), (TOP, 0), (TOP, 5), (TOP, TOP), (0, TOP)):
        end = in_base + n_in
        for lo in sorted({-2 ** 40, -7, -1, 0, 1, in_base - 1, in_base, in_base + 1, end - 1, end}):
            for hi in sorted({lo, lo + 1, 0, in_base, end - 1, end, end + 1}):
                if hi >= lo and -2 ** 63 <= lo and hi < 2 ** 63:
                    cases.append((in_base, n_in, lo, hi))
    got = _run([a for c in cases for a in ("w",) + c])
    assert len(got) == len(cases)
    seen = set()
    for (in_base, n_in, lo, hi), (ok, need_lo, length) in zip(cases, got):
        want_lo = max(lo, 0)
        want = (int(want_lo >= in_base and hi <= in_base + n_in), want_lo, max(hi - want_lo, 0))
        assert (ok, need_lo, length) == want, (in_base, n_in, lo, hi, (ok, need_lo, length), want)
        for name, hit in (("lo < 0", lo < 0), ("lo < in_base", 0 <= lo < in_base), ("hi == end", hi == in_base + n_in), ("hi == end + 1", hi == in_base + n_in + 1),
                          ("n_in == 0", n_in == 0), ("in_base == 2^62 - 1", in_base == TOP)):
            if hit:
                seen.add((name, ok))
    # every named edge was met, and with both verdicts where both exist (one sample past the end is always refused)
    assert seen == {(n, v) for n in ("lo < 0", "hi == end", "n_in == 0", "in_base == 2^62 - 1") for v in (0, 1)} | {("lo < in_base", 0), ("hi == end + 1", 0)}

"""Inputs of the re-acquisition tests (CPU and GPU): six-subframe spans that carry one PSS at a known place, the drifting recording of track_cases cut in three
ways - samples removed, samples duplicated -, and the float64 replay that brings a cut recording back with the model loop and the rule of DESIGN 3.1k."""
import functools

import numpy as np

import reacq_model as rq
import track_model as tm
from track_cases import DRIFT_LEAD, drifting_recording, pss_subframe, rep, sinc_at

# where the recording is cut (input sample, counted from the recording's first) and how: samples removed (negative) or duplicated (positive); the offsets the
# search must find are the cut times 96 / 125 output samples, on the d grid (d = 4 at N = 512)
CUT_AT = DRIFT_LEAD + 200000
CUTS = {"removed_3000": -3000, "removed_17001": -17001, "duplicated_9000": 9000}
CUT_OFFSETS = {"removed_3000": -2304, "removed_17001": -13056, "duplicated_9000": 6912}
CUT_AFTER, CUT_PPM = 4, 60.0
# what the model round trip gives for all three (tests/test_reacq_model.py asserts it): the search runs at segment 9, the jump is in force at segment 12
CUT_SEARCH_SEGMENT, CUT_JUMP_SEGMENT = 9, 12


def span(N, ats, nant=1, snr_db=30.0, cfo_hz=0.0, noise=0.05, seed=3):
    """[6][nant][15 N] complex64: noise, and for every `at` in ats (floats, at least 15 N apart) one PSS subframe of track_cases added so that its PSS symbol's
    useful part starts at sample `at` of the span (the subframe's samples that fall outside the span are dropped).  Antenna a: another realisation at 0.7^a"""
    sflen = 15 * N
    rng = np.random.default_rng(seed + N)
    out = (noise * (rng.standard_normal((nant, 6 * sflen)) + 1j * rng.standard_normal((nant, 6 * sflen)))).astype(np.complex64)
    for at in ats:
        whole = int(np.floor(at))
        first = whole - tm.pss_index(N)                    # where the subframe's sample 0 lands
        for a in range(nant):
            sf = pss_subframe(N, float(at) - whole, snr_db, cfo_hz, seed=1 + 17 * a) * np.float32(0.7 ** a)
            lo, hi = max(first, 0), min(first + sflen, 6 * sflen)
            out[a, lo:hi] += sf[lo - first:hi - first]
    return np.ascontiguousarray(out.reshape(nant, 6, sflen).transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def cut_recording(name):
    """the drifting recording [sample][antenna] complex64 with CUTS[name] applied at CUT_AT, read-only"""
    f = drifting_recording()[5]
    n = CUTS[name]
    g = np.concatenate([f[:CUT_AT], f[CUT_AT - n:]] if n < 0 else [f[:CUT_AT], f[CUT_AT - n:CUT_AT], f[CUT_AT:]])
    g.setflags(write=False)
    return g


def model_replay(f, rate_in, nsf, initial_ppm=0.0, after=None, min_ratio=rq.MIN_RATIO, n_id_2=1, N=512, lead=DRIFT_LEAD, probe=()):
    """track_cases.model_replay with the rule of DESIGN 3.1k on top (after = None: without it) -> ([nsf][antenna][15 N] complex64, per-segment log of
    (valid, e, invalid_run behind the loop step), the searches [(segment, accepted, o, peak, ratio)], the jumps [(segment in force, o)]).  probe: segments whose span
    is searched as well, for the figures only - they join the list of searches behind the real ones and change nothing"""
    from fractions import Fraction
    sflen, seglen = 15 * N, 75 * N
    rate_out = 15000.0 * N
    d_nom = int(round(Fraction(int(rate_in)) / Fraction(int(rate_out)) * (1 << 64)))
    d, p, r = tm.lag_spacing(N), tm.pss_index(N), rep(N, 0.0, n_id_2)
    out = np.zeros((nsf, f.shape[1], sflen), dtype=np.complex64)
    state, peaks = tm.new_state(initial_ppm, seglen), tm.Peaks()
    rule = rq.Rule(after) if after is not None else None
    base, meas, log, searches, jumps, seg, hist_after = lead << 64, [], [], [], [], {}, []

    def at(b, step, n):
        return (b >> 64) + float(b & ((1 << 64) - 1)) * 2.0 ** -64 + np.arange(n, dtype=np.float64) * (float(step) * 2.0 ** -64)

    def search(h0):
        b, step = seg[h0]
        y = sinc_at(f, at(b, step, 6 * sflen)).astype(np.complex64)
        x = y.reshape(6, sflen, -1).transpose(0, 2, 1)
        mean, hist = None, hist_after[h0 + 1]           # the history behind the measurement of segment h0 + 1: what the library has when it enters h0 + 3
        if hist:
            s = 0.0
            for v in hist:
                s = s + v
            mean = s / len(hist)
        res = rq.decide(rq.metric(x, r, d), d, N, min_ratio, mean)
        searches.append((h0,) + res)
        return res

    for h in range(nsf // 5):
        if h < tm.DELAY:
            step = d_nom + tm.delta_of(state["correction"], rate_in, rate_out, seglen)
        else:
            ok, e = meas[h - tm.DELAY]
            state, delta = tm.loop_step(state, e, ok, rate_in, rate_out, seglen)
            step = d_nom + delta
        if rule is not None:
            jump, state["invalid_run"], _ = rule.entered(h, state["invalid_run"], search)
            if jump is not None:
                base += jump * seg[h - rq.DELAY][1]          # o outputs at the step of the segment that was searched, exact
                jumps.append((h, jump))
        seg[h] = (base, step)
        y = sinc_at(f, at(base, step, seglen)).astype(np.complex64)
        out[5 * h:5 * h + 5] = y.reshape(5, sflen, -1).transpose(0, 2, 1)
        ok, e, peak = tm.observe(tm.corr13(out[5 * h], p, r, d), d)
        ok = ok and peaks.accept(peak)
        meas.append((ok, e if ok else 0.0))
        hist_after.append(list(peaks.hist))
        log.append((ok, e, state["invalid_run"]))
        base += seglen * step
    for h0 in probe:
        search(h0)
    return out, log, searches, jumps

"""Shared by the tests of a live stream with the channel filter on (CPU: test_stream_filter_plan.py, GPU: test_gpu_stream_filter.py): the cell sets
the plan is checked on, the composition of the existing span helpers a filtered stream's plan must equal, and the float64 chain - chanfilt_model stage 1, then the
model detector and loop of track_model around the float64 sampler of track_cases - that establishes what a tracked, filtered stream has to decode."""
import functools

import numpy as np

import ltesniffer_amd as la
import track_model as tm
from chanfilt_cases import RATE, STOP
from resample_model import passband_hz

SF = {100: 30720, 75: 23040, 50: 15360, 25: 7680}   # output samples of one subframe (3GPP rates)
LEAD = 1000
# set 1: the two 100-PRB cells at +-9.9 MHz of 61.44 MS/s with S = STOP (L = 88), 12 subframes; set 2: a 75- next to a 25-PRB cell of 30.72 MS/s with
# cells_stopbands' values (cells_cases: 20 subframes, the 25-PRB cell cut by max_subframes)
TWO = (RATE, LEAD + 12 * 61440 + 1000, [dict(nof_prb=100, center_offset_hz=9.9e6, offset_time=LEAD), dict(nof_prb=100, center_offset_hz=-9.9e6, offset_time=LEAD)],
       [STOP, STOP])
MIXED_CELLS = [dict(nof_prb=75, center_offset_hz=-4.5e6, offset_time=LEAD), dict(nof_prb=25, center_offset_hz=7.5e6, offset_time=LEAD, max_subframes=20)]


def mixed():
    stops = la.cells_stopbands([c["center_offset_hz"] for c in MIXED_CELLS], [c["nof_prb"] for c in MIXED_CELLS], 30.72e6)
    return 30.72e6, LEAD + 20 * 30720 + 1000, MIXED_CELLS, stops


def half_len(rate_in, c, S):
    return la.channel_filter_design(rate_in, passband_hz(c["nof_prb"]), S)["L"]


def wide_span(rate_in, c, S, sf0, nsf):
    """the input samples [lo, hi) stage 1 reads for subframes [sf0, sf0 + nsf) of the cell: the resampler's span (clamped at sample 0, as the file pass's), then
    the filter's span of exactly those y1 - the composition of the two existing span helpers.  lo is not clamped"""
    n, B = SF[c["nof_prb"]], passband_hz(c["nof_prb"])
    sp = la.resample_span(nsf * n, 10 ** 12, rate_in, 1000.0 * n, first_sample=c.get("offset_time", 0), out_first=sf0 * n, passband_hz=B)
    lo = max(sp["in_lo"], 0)
    w = la.channel_filter_span(sp["in_hi"] - lo, 10 ** 12, rate_in, B, S, out_first=lo, center_offset_hz=c.get("center_offset_hz", 0.0))
    assert w["taps"] == 2 * half_len(rate_in, c, S) + 1
    return w["in_lo"], w["in_hi"]


def complete(rate_in, c, S, pushed):
    """complete subframes of the cell after `pushed` samples: the y1 those samples carry, then the outputs whose taps lie inside that y1"""
    n, B = SF[c["nof_prb"]], passband_hz(c["nof_prb"])
    y_end = la.channel_filter_span(0, pushed, rate_in, B, S, center_offset_hz=c.get("center_offset_hz", 0.0))["max_out"]
    k = la.resample_span(0, y_end, rate_in, 1000.0 * n, first_sample=c.get("offset_time", 0), passband_hz=B)["max_out"] // n
    return min(k, c["max_subframes"]) if c.get("max_subframes") else k


# ---- the float64 chain of a tracked, filtered stream ----

def model_track_replay(y1, rate_in, N, nsf, tti0, n_id_2, lead, initial_ppm=0.0):
    """y1 [sample][antenna] (stage 1's output from sample 0 on, float64) resampled to 15 kHz N segment by segment by the float64 sampler of track_cases with the
    model detector and the model loop at the loop's two-segment delay, the segments anchored at the TTIs that are multiples of 5 (segment 0 may be shorter and then
    has no PSS; the last may be cut) -> ([nsf][antenna][15 N] complex64, the per-segment log (valid, e, correction in ppm))"""
    from fractions import Fraction
    from track_cases import rep, sinc_at
    sflen, seglen = 15 * N, 75 * N
    rate_out = 15000.0 * N
    d_nom = int(round(Fraction(int(rate_in)) / Fraction(int(rate_out)) * (1 << 64)))
    d, p, r = tm.lag_spacing(N), tm.pss_index(N), rep(N, 0.0, n_id_2)
    out = np.zeros((nsf, y1.shape[1], sflen), dtype=np.complex64)
    state, peaks = tm.new_state(initial_ppm, seglen), tm.Peaks()
    base, meas, log, sf0, h = lead << 64, [], [], 0, 0
    while sf0 < nsf:
        n = min((5 - tti0 % 5) if h == 0 else 5, nsf - sf0)
        if h < tm.DELAY:
            step = d_nom + tm.delta_of(state["correction"], rate_in, rate_out, seglen)
        else:
            ok, e = meas[h - tm.DELAY]
            state, delta = tm.loop_step(state, e, ok, rate_in, rate_out, seglen)
            step = d_nom + delta
        t = (base >> 64) + float(base & ((1 << 64) - 1)) * 2.0 ** -64 + np.arange(n * sflen, dtype=np.float64) * (float(step) * 2.0 ** -64)
        y = sinc_at(y1, t).astype(np.complex64)
        out[sf0:sf0 + n] = y.reshape(n, sflen, -1).transpose(0, 2, 1)
        ok, e = False, 0.0
        if h or tti0 % 5 == 0:     # the segment's first subframe carries a PSS
            ok, e, peak = tm.observe(tm.corr13(out[sf0], p, r, d), d)
            ok = ok and peaks.accept(peak)
        meas.append((ok, e if ok else 0.0))
        log.append((ok, e, state["correction"] / seglen * 1e6))
        base += n * sflen * step
        sf0 += n
        h += 1
    return out, log


@functools.lru_cache(maxsize=None)
def chain_strong_neighbour():
    """case (a): both cells of the 61.44 MS/s recording whose other carrier is 20 dB stronger (chanfilt_cases.recording), the clock right, the loop on.
    -> [(sc, tti0, options, oracle records, the chain's records, the loop's log)] for the weak cell B and the strong cell A"""
    from chanfilt_cases import B100, NSF, recording
    from chanfilt_model import Design
    from parity import oracle_records, run_oracle
    f = recording("b_wanted")[-1]                     # B at amplitude 1, A at amplitude 10: one recording, two cells
    m = Design(RATE, B100, STOP)
    out = []
    for case in ("b_wanted", "a_wanted"):
        sc, tti0, orecs, _, opt, rate_in, native, f0, _ = recording(case)
        x = f.astype(np.complex64).astype(np.complex128)
        y1 = m.apply(x, 0, 0, m.max_out(len(x)), f0)
        iq, log = model_track_replay(y1, rate_in, 2048, NSF, tti0, sc["cell_id"] % 3, LEAD)
        recs = oracle_records(run_oracle(sc, tti0, iq, taps=False, **opt)[2])
        out.append((sc, tti0, opt, orecs, recs, log))
    return out


DRIFT_STOP = 3.5e6     # the drifting 25-PRB recording at 10 MS/s: L = 21


@functools.lru_cache(maxsize=None)
def chain_drifting():
    """case (b): track_cases.drifting_recording with S = 3.5 MHz and initial_ppm = 60 -> (oracle records, the chain's records, the loop's log)"""
    from chanfilt_model import Design
    from parity import oracle_records, run_oracle
    from track_cases import DRIFT_LEAD, DRIFT_NSF, drifting_recording
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    m = Design(rate, passband_hz(25), DRIFT_STOP)
    assert m.L == 21 and tti0 % 5 == 0
    y1 = m.apply(f.astype(np.complex128), 0, 0, m.max_out(len(f)))
    iq, log = model_track_replay(y1, rate, 512, DRIFT_NSF, tti0, sc["cell_id"] % 3, DRIFT_LEAD, initial_ppm=60.0)
    return orecs, oracle_records(run_oracle(sc, tti0, iq, taps=False, **opt)[2]), log

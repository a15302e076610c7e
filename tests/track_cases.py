"""Inputs of the timing-loop tests (CPU and GPU): single subframes that carry a PSS at a known, fractional place - cut out of clock_cases.pss_train, the exact
continuous-time synthesis with a loaded neighbourhood - in the block-buffer layout [subframe][antenna][sample]; and a 400-subframe recording made by a clock that is
off and slews, sampled in float64 at the clock's own instants, with the float64 replay (open loop, or with the model loop) that brings it back."""
import functools

import numpy as np

from clock_cases import pss_train
from clock_model import replica
from track_model import pss_index

# the detector cases of the issue: N, (snr_db, cfo_hz), true offsets in units of d spread over +-4 d, fractions included
DETECT_N = (128, 512, 2048)
DETECT_CHANNELS = ((30.0, 0.0), (10.0, 0.0), (30.0, 2000.0), (10.0, 2000.0))
DETECT_OFFSETS = (-4.0, -2.5, -1.3, -0.5, 0.0, 0.37, 1.75, 3.2, 4.0)


@functools.lru_cache(maxsize=None)
def pss_subframe(N, offset, snr_db=30.0, cfo_hz=0.0, seed=1, n_id_2=1):
    """one subframe (15 N samples, complex64, read-only) whose PSS symbol's useful part starts `offset` samples (a float) behind pss_index(N): the train's second
    subframe, so that the loaded symbol in front of the PSS is whole"""
    sflen = 15 * N
    x, _ = pss_train(N, 1, 0.0, snr_db, cfo_hz, n_id_2=n_id_2, seed=seed, u0=float(sflen + pss_index(N)) + float(offset))
    sf = np.ascontiguousarray(x[sflen:2 * sflen])
    assert sf.shape == (sflen,)
    sf.setflags(write=False)
    return sf


def rep(N, cfo_hz=0.0, n_id_2=1):
    """the replica the library forms for a cfo_hz given as a float"""
    return replica(n_id_2, N, float(np.float32(cfo_hz)))


def blocks(N, offsets, nant=1, snr_db=30.0, cfo_hz=0.0):
    """[len(offsets)][nant][15 N] complex64: subframe i carries its PSS at offsets[i] (None: a subframe of zeros); antenna a is another noise and load realisation
    of the same timing, at 0.7^a of the amplitude"""
    out = np.zeros((len(offsets), nant, 15 * N), dtype=np.complex64)
    for i, off in enumerate(offsets):
        if off is None:
            continue
        for a in range(nant):
            out[i, a] = pss_subframe(N, float(off), snr_db, cfo_hz, seed=1 + 17 * a) * np.float32(0.7 ** a)
    return out


# ---- a recording made by a clock that is off and slews (the reason for the loop) ----
DRIFT_STREAM, DRIFT_NSF = "prb25_2port", 400        # the narrowest scenario of srs_streams: 25 PRB, N = 512, 7.68 MS/s, two antennas; 80 segments
DRIFT_RATE = 10.0e6                                 # the recording's nominal rate: not the engine's (D = 125 / 96)
DRIFT_PPM0, DRIFT_SLEW = 60.0, 20.0                 # the clock is off by 60 ppm at the start and by 80 ppm at the end
DRIFT_LEAD, DRIFT_TAIL = 1000, 3000                 # samples of the recording in front of and behind the capture (its periodic continuation)


def sinc_at(x, t, half=16):
    """x[n, ...] at the instants t (float64, in samples of x; every t - half >= 0 and t + half + 1 < len(x)): a direct float64 sinc sum under a 4-term
    Blackman-Harris window of 2 half + 1 samples - resample_cases.sinc_convert at arbitrary instants.  half = 16: the window's main lobe is 8 / 33 of the rate
    wide, so everything below 0.38 of the rate passes and images fold from above 0.62 - the 25-PRB signal reaches 0.30 of the engine's rate and 0.23 of the
    recording's"""
    x = np.asarray(x, dtype=np.complex128)
    t = np.asarray(t, dtype=np.float64)
    out = np.zeros(t.shape + x.shape[1:], dtype=np.complex128)
    j = np.arange(-half, half + 1)
    sign = np.where(j % 2 == 0, 1.0, -1.0)
    cj, sj = np.cos(np.pi * j / (half + 1)), np.sin(np.pi * j / (half + 1))
    for c0 in range(0, len(t), 32768):
        tt = t[c0:c0 + 32768]
        n0 = np.floor(tt).astype(np.int64)
        assert n0.min() - half >= 0 and n0.max() + half < x.shape[0]
        fr = tt - n0
        d = fr[:, None] - j[None, :]                        # distance to sample n0 + j, |d| < half + 1
        # sin(pi (fr - j)) = (-1)^j sin(pi fr) and cos(pi (fr - j) / (half + 1)) by the addition theorem: no transcendental function on the big arrays
        near = np.abs(d) < 1e-9
        c = (np.sin(np.pi * fr)[:, None] * sign[None, :]) / (np.pi * np.where(near, 1.0, d))
        c[near] = 1.0
        c1 = np.cos(np.pi * fr / (half + 1))[:, None] * cj[None, :] + np.sin(np.pi * fr / (half + 1))[:, None] * sj[None, :]
        c *= 0.35875 + 0.48829 * c1 + 0.14128 * (2.0 * c1 * c1 - 1.0) + 0.01168 * ((4.0 * c1 * c1 - 3.0) * c1)
        xs = x[n0[:, None] + j[None, :]]
        out[c0:c0 + len(tt)] = np.einsum("ij,ij...->i...", c, xs)
    return out


@functools.lru_cache(maxsize=None)
def drifting_recording():
    """computed once, shared, read-only -> (sc, tti0, the oracle's records of the native stream, options, the recording's nominal rate, the recording [sample][antenna]
    complex64 whose sample DRIFT_LEAD is the first sample of the stream).  Recording sample n (counted from DRIFT_LEAD) was taken by a clock that runs at
    DRIFT_RATE (1 + eps(n)), eps(n) = (DRIFT_PPM0 + DRIFT_SLEW n / n_total) 1e-6: at native time u(n) = (fs / R) (ln(1 + a + b n) - ln(1 + a)) / b, exactly the
    integral of dn / (1 + eps(n))"""
    from resample_cases import native_stream
    sc, tti0, iq, orecs, _, opt = native_stream(DRIFT_STREAM, DRIFT_NSF)
    native = 15000.0 * 512
    x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, iq.shape[1]).astype(np.complex128)      # [sample][antenna]
    pad = 4096
    xp = np.concatenate([x[-pad:], x, x[:pad]])                                                             # the periodic continuation on both sides
    n_total = int(np.ceil(len(x) * DRIFT_RATE / native * (1.0 + 1e-4)))
    a, b = DRIFT_PPM0 * 1e-6, DRIFT_SLEW * 1e-6 / n_total
    n = np.arange(-DRIFT_LEAD, n_total + DRIFT_TAIL, dtype=np.float64)
    u = (native / DRIFT_RATE) * (np.log1p(a + b * n) - np.log1p(a)) / b
    assert u[0] > -pad + 40 and u[-1] < len(x) + pad - 40 and u[-1] > len(x)
    f = sinc_at(xp, u + pad).astype(np.complex64)
    f.setflags(write=False)
    return sc, tti0, orecs, opt, DRIFT_RATE, f


def record_tti(rec):
    """the TTI in the context header of a MAC-LTE record (mac_lte_record: tag 4, system frame number << 4 | subframe)"""
    fs = (rec[10] << 8) | rec[11]
    return (fs >> 4) * 10 + (fs & 15)


def model_replay(f, rate_in, nsf, track=True, initial_ppm=0.0, n_id_2=1, N=512, lead=DRIFT_LEAD):
    """the recording brought back to the engine's rate by the float64 sampler - open loop at the nominal rate (track = False), or segment by segment with the model
    detector and the model loop, at the loop's two-segment delay -> ([nsf][antenna][15 N] complex64, the list of per-segment (valid, e, correction in ppm))"""
    import track_model as tm
    from fractions import Fraction
    sflen, seglen = 15 * N, 75 * N
    rate_out = 15000.0 * N
    ratio = Fraction(int(rate_in)) / Fraction(int(rate_out))
    d_nom = int(round(ratio * (1 << 64)))      # D = round(rate_in / rate_out 2^64), exactly
    d, p, r = tm.lag_spacing(N), tm.pss_index(N), rep(N, 0.0, n_id_2)
    out = np.zeros((nsf, f.shape[1], sflen), dtype=np.complex64)
    state, peaks = tm.new_state(initial_ppm if track else 0.0, seglen), tm.Peaks()
    base, meas, log = lead << 64, [], []
    for h in range(nsf // 5):
        if h < tm.DELAY or not track:
            step = d_nom + tm.delta_of(state["correction"], rate_in, rate_out, seglen)
        else:
            ok, e = meas[h - tm.DELAY]
            state, delta = tm.loop_step(state, e, ok, rate_in, rate_out, seglen)
            step = d_nom + delta
        t = (base >> 64) + float(base & ((1 << 64) - 1)) * 2.0 ** -64 + np.arange(seglen, dtype=np.float64) * (float(step) * 2.0 ** -64)
        y = sinc_at(f, t).astype(np.complex64)                                      # [seglen][antenna]
        out[5 * h:5 * h + 5] = y.reshape(5, sflen, -1).transpose(0, 2, 1)
        ok, e, peak = tm.observe(tm.corr13(out[5 * h], p, r, d), d)
        ok = ok and peaks.accept(peak)
        meas.append((ok, e if ok else 0.0))
        log.append((ok, e, state["correction"] / seglen * 1e6))
        base += seglen * step
    return out, log

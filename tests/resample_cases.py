"""Shared by the resampler tests (CPU and GPU): the rate pairs, tones whose value at any instant is known exactly, the independent conversions of a
3GPP-rate capture to a foreign rate (whole-capture FFT zero-padding / truncation; a direct sinc sum for the ppm pair), and the streams of
srs_streams.STREAMS that are decoded after the round trip."""
import math

import numpy as np

from resample_model import Plan, passband_hz

PPM = 150e-6
# (rate_in, rate_out, nof_prb)
PAIRS = [(20e6, 30.72e6, 100), (25e6, 30.72e6, 100), (61.44e6, 30.72e6, 100), (12.5e6, 15.36e6, 50), (25e6, 23.04e6, 100),
         (7.68e6 * (1 + PPM), 7.68e6, 25), (7.68e6 * (1 - PPM), 7.68e6, 25)]
FAR = 20_000_000_000   # a first_sample ten minutes into a 30.72 MS/s recording
Q = 4096               # tones sit at rate_in * k / Q: their phase at input sample n is (k n mod Q) / Q, exact in integers


def tone(k, n_lo, n_hi):
    """exp(2 pi j k n / Q) for n_lo <= n < n_hi (zero for n < 0, as the resampler reads the recording)"""
    n = np.arange(n_lo, n_hi, dtype=np.int64)
    x = np.exp(2j * np.pi * ((k * n) % Q) / Q)
    x[n < 0] = 0.0
    return x


def tone_at(k, positions):
    """the same tone at 64.64 positions (Python integers): exact phase reduction before the float64 exponential"""
    mod = Q << 64
    return np.exp(2j * np.pi * np.array([((k * p) % mod) / mod for p in positions], dtype=np.float64))


def fold(f, rate):
    return f - rate * np.round(f / rate)


def passband_tones(rate_in, nof_prb):
    """k of tones inside |f| <= B, the edges included (the grid point nearest to the edge from inside)"""
    B = passband_hz(nof_prb)
    kmax = int(math.floor(B / rate_in * Q))
    return sorted({-kmax, -kmax // 2, -3, 0, 1, kmax // 3, kmax - 1, kmax})


def landing_tones(rate_in, rate_out, nof_prb, step=37):
    """[(k, f_landing)]: input tones outside the pass band, one component of which (the tone itself after folding at rate_out, or one of its images at
    f + i rate_in) lands inside the occupied band of the output"""
    B = passband_hz(nof_prb)
    out = []
    ks = list(range(-Q // 2, Q // 2, step))
    kb = int(math.ceil(B / rate_in * Q))   # the tones nearest to the stop-band edges, where the filter is weakest
    for s in (-1, 1):
        e = s * (min(rate_in, rate_out) - B) / rate_in * Q
        ks += [int(math.floor(e)), int(math.ceil(e))]
    for k in sorted(set(ks)):
        if abs(k) <= kb or abs(k) > Q // 2:
            continue
        f = rate_in * k / Q
        for i in range(-5, 6):
            F = f + i * rate_in
            fl = float(fold(F, rate_out))
            if abs(fl) <= B and (i != 0 or abs(F) > rate_out / 2):
                out.append((k, fl))
    return out


def window(n):
    """4-term Blackman-Harris (side lobes 92 dB down): weights of the amplitude estimates"""
    a = 2 * np.pi * np.arange(n) / (n - 1)
    return 0.35875 - 0.48829 * np.cos(a) + 0.14128 * np.cos(2 * a) - 0.01168 * np.cos(3 * a)


def amplitude_at(y, f_hz, rate_out):
    """amplitude of the component of y at f_hz"""
    w = window(len(y))
    return float(abs(np.sum(w * y * np.exp(-2j * np.pi * f_hz / rate_out * np.arange(len(y))))) / np.sum(w))


def check_tones(resample_fn, rate_in, rate_out, nof_prb, first_sample=0, first_frac=0.3, n_out=3000):
    """-> (worst pass-band error, relative RMS; worst amplitude landing in the occupied band).  resample_fn(plan, x, in_base, n_out) -> y[n_out]"""
    plan = Plan(rate_in, rate_out, passband_hz(nof_prb), first_sample, first_frac)
    lo, hi = plan.span(0, n_out)
    pos = [plan.position(m) for m in range(n_out)]
    skip = plan.taps if lo < 0 else 0     # the outputs that read the zeros in front of the recording are not a tone's
    worst_pass, worst_land = 0.0, 0.0
    for k in passband_tones(rate_in, nof_prb):
        y = resample_fn(plan, tone(k, max(lo, 0), hi), max(lo, 0), n_out)
        ref = tone_at(k, pos)
        e = np.sqrt(np.sum(np.abs(y[skip:] - ref[skip:]) ** 2) / np.sum(np.abs(ref[skip:]) ** 2))
        worst_pass = max(worst_pass, float(e))
    for k, fl in landing_tones(rate_in, rate_out, nof_prb):
        y = resample_fn(plan, tone(k, max(lo, 0), hi), max(lo, 0), n_out)
        worst_land = max(worst_land, amplitude_at(y[skip:], fl, rate_out))
    return worst_pass, worst_land


# ---- a 3GPP-rate capture at a foreign rate, by methods that share nothing with the product's filter ----
def fft_convert(x, num, den):
    """x[n, ...] (axis 0: samples; periodic) -> [n num / den, ...]: the whole capture's spectrum zero-padded or truncated, float64"""
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[0]
    assert (n * num) % den == 0
    m = n * num // den
    X = np.fft.fft(x, axis=0)
    keep = min(n, m)
    h = keep // 2
    Y = np.zeros((m,) + x.shape[1:], dtype=np.complex128)
    Y[:h] = X[:h]
    Y[m - h:] = X[n - h:]
    return np.fft.ifft(Y, axis=0) * (m / n)


def sinc_convert(x, ratio, k_lo, k_hi, half=96):
    """x[n, ...] (periodic) at times k * ratio (in samples of x), k_lo <= k < k_hi: a direct float64 sinc sum under a 4-term Blackman-Harris window of
    2 * half + 1 samples (the product's filter is a Kaiser window of at most 192 taps)"""
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[0]
    out = np.zeros((k_hi - k_lo,) + x.shape[1:], dtype=np.complex128)
    j = np.arange(-half, half + 1)
    for c0 in range(k_lo, k_hi, 16384):
        c1 = min(k_hi, c0 + 16384)
        t = np.arange(c0, c1, dtype=np.float64) * ratio
        n0 = np.floor(t).astype(np.int64)
        d = (t - n0)[:, None] - j[None, :]                    # distance to sample n0 + j
        a = np.pi * d / (half + 1)
        w = 0.35875 + 0.48829 * np.cos(a) + 0.14128 * np.cos(2 * a) + 0.01168 * np.cos(3 * a)
        w[np.abs(d) > half + 1] = 0.0
        c = np.sinc(d) * w
        xs = x[(n0[:, None] + j[None, :]) % n]
        out[c0 - k_lo:c1 - k_lo] = np.sum(c.reshape(c.shape + (1,) * (x.ndim - 1)) * xs, axis=1)
    return out


LEAD, TAIL = 1000, 1000   # samples of the file's rate in front of and behind the capture (its periodic continuation)

# name -> (stream of srs_streams.STREAMS, subframes (None: the stream's own), file rate as (num, den) of the 3GPP rate or a ppm factor)
CASES = {
    "prb100_from_20": ("prb100_tm34_256qam", None, (125, 192)),
    "prb100_from_25": ("prb100_tm34_256qam", None, (625, 768)),
    "prb100_from_61p44": ("prb100_tm34_256qam", None, (2, 1)),
    "prb50_from_12p5": ("prb50_1port_extcp", None, (625, 768)),
    "prb25_plus_150ppm": ("prb25_2port", 48, 1 + PPM),
    "prb25_minus_150ppm": ("prb25_2port", 48, 1 - PPM),
}


def native_stream(name, nsf=None):
    """srs_streams.stream, optionally with another number of subframes of the same scenario (the ppm pair needs >= 40)"""
    import srs_streams as S
    from lsn_testlib import oracle_trace, scenario
    from parity import gen_subframes, oracle_records, run_oracle
    if nsf is None:
        return S.stream(name)
    preset, _, over, opt = S.STREAMS[name]
    sc = scenario(preset, **over)
    tti0, iq, _ = gen_subframes(sc, nsf)
    _, _, orecs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
    return sc, tti0, iq, oracle_records(orecs), oracle_trace(), opt


def foreign_capture(case):
    """-> (sc, tti0, oracle records at the 3GPP rate, oracle trace, options, rate_in, rate_native, file samples [sample][antenna] complex128).
    Sample LEAD of the file is the first sample of the capture; the file continues the capture periodically on both sides."""
    from rate_convert import SYMBOL_SZ_3GPP
    name, nsf, how = CASES[case]
    sc, tti0, iq, orecs, otrace, opt = native_stream(name, nsf)
    native = 15000.0 * SYMBOL_SZ_3GPP[sc["nof_prb"]]
    x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, iq.shape[1])   # [sample][antenna]
    if isinstance(how, tuple):
        y = fft_convert(x, *how)
        rate_in = native * how[0] / how[1]
        f = np.concatenate([y[len(y) - LEAD:], y, y[:TAIL]])
    else:
        rate_in = native * how
        n = int(math.ceil(x.shape[0] * how))
        f = sinc_convert(x, 1.0 / how, -LEAD, n + TAIL)
    return sc, tti0, orecs, otrace, opt, rate_in, native, f

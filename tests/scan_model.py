"""Float64 model of the carrier scan, written from the definition in DESIGN.md section 3.1d (not from the kernels or lsn_scan.cc), and the recordings the CPU
and GPU tests of the scan share.

Hypotheses: f_k = float(k) * raster_hz + raster_offset_hz for every integer k with |f_k| + B6 <= rate_in / 2, B6 = 15 kHz * 37, optionally f_lo <= f_k <= f_hi;
tuning word of f_k: ddc_cases.tuning_word.
Channel: the resampler of section 3.1b (resample_model.Plan: positions, bank, H + f dH) from rate_in to 1.92 MS/s with pass band B6, output 0 at input 0, the
ratio allowed up to 64 and the Kaiser estimate up to 768 taps; in front of it the exact-phase mixer ddc_cases.mix.
Metric: C[r][n] = sum_q |sum_k y[q W5 + n + k] conj(p_r[k])|^2 / sum_k |y[q W5 + n + k]|^2 over q < P (N = 128, W5 = 9600, p_r = clock_model.replica(r, 128));
peak = the first maximum in (root, lag) order, p2avg = peak / mean_n C[root of the peak][n].
Decision: p2avg >= threshold and peak >= threshold P / N, sorted by metric descending (ties: lower |f_k|, then lower k), accepted greedily, dropped when strictly closer than
min_spacing_hz to an accepted one."""
import functools
import math
from fractions import Fraction

import numpy as np

from ddc_cases import mix, tuning_word
from resample_model import ATTEN_DB, PHASES, Plan

RATE_OUT = 1.92e6
B6 = 15000.0 * 37
N, W5 = 128, 9600
MAX_RATIO, MAX_TAPS, MAX_HYPOTHESES = 64.0, 768, 8192


class ChannelPlan(Plan):
    """resample_model.Plan for rate_in -> 1.92 MS/s, pass band B6, with the two caps of the carrier scan instead of the resampler's (4 and 192); positions, spans,
    phases and the filter sum are the parent's"""

    def __init__(self, rate_in, first_sample=0, first_frac=0.0):
        rate_in = float(rate_in)
        self.rate_in, self.rate_out = rate_in, RATE_OUT
        if not RATE_OUT <= rate_in <= MAX_RATIO * RATE_OUT:
            raise ValueError("outside the accepted range")
        self.step = int((2 * Fraction(rate_in) / Fraction(RATE_OUT) * 2 ** 64 + 1) // 2)
        self.start = (int(first_sample) << 64) + int(Fraction(first_frac) * 2 ** 64)
        self.rho = rate_in / RATE_OUT
        width = (RATE_OUT - 2.0 * B6) / rate_in
        want = (ATTEN_DB - 7.95) / (14.36 * width) + 1.0
        if want > MAX_TAPS:
            raise ValueError("outside the accepted range")
        self.taps = T = max(4, 2 * int(math.ceil(want / 2.0)))
        beta = 0.1102 * (ATTEN_DB - 8.7)
        t = np.arange(T)[None, :] - T / 2 + 1 - np.arange(PHASES + 1)[:, None] / PHASES
        u = np.clip(1.0 - (2.0 * t / T) ** 2, 0.0, None)
        self.H = np.sinc(t / self.rho) / self.rho * np.i0(beta * np.sqrt(u)) / np.i0(beta)
        self.H[np.abs(t) > T / 2] = 0.0


def hypotheses(rate_in, raster_hz=100e3, raster_offset_hz=0.0, f_lo_hz=None, f_hi_hz=None):
    """-> [(k, f_k)] in ascending k; ValueError for none or more than 8192"""
    rate_in, raster_hz, raster_offset_hz = float(rate_in), float(raster_hz), float(raster_offset_hz)
    kmax = int(math.ceil(0.5 * rate_in / raster_hz + abs(raster_offset_hz) / raster_hz)) + 2
    if kmax > 4 * MAX_HYPOTHESES:
        raise ValueError("too many hypotheses")
    out = []
    for k in range(-kmax, kmax + 1):
        f = float(k) * raster_hz + raster_offset_hz
        if abs(f) + B6 <= rate_in / 2 and (f_lo_hz is None or f_lo_hz <= f <= f_hi_hz):
            out.append((k, f))
    if not out or len(out) > MAX_HYPOTHESES:
        raise ValueError("no hypothesis, or more than %d" % MAX_HYPOTHESES)
    return out


def channel_samples(nof_periods):
    return (nof_periods + 1) * W5 + N


def channel(x, rate_in, f_hz, n_out, m0=0, in_base=0, first_sample=0, first_frac=0.0, with_bound=False):
    """x[sample] or x[sample][antenna], x[0] = sample in_base of the recording -> outputs m0 .. m0 + n_out - 1 of the channel of offset f_hz, complex128"""
    plan = ChannelPlan(rate_in, first_sample, first_frac)
    return plan.apply(mix(x, in_base, tuning_word(f_hz, rate_in)), m0, n_out, in_base=in_base, with_bound=with_bound)


@functools.lru_cache(maxsize=None)
def _replicas():
    from clock_model import replica
    return np.stack([replica(r, N).astype(np.complex128) for r in range(3)])


def correlate(y, nof_periods):
    """y: channel samples, at least (P + 1) W5 + N -> C[3][W5] float64"""
    y = np.asarray(y, dtype=np.complex128)
    p = _replicas()
    C = np.zeros((3, W5))
    for q in range(nof_periods):
        win = np.lib.stride_tricks.sliding_window_view(y[q * W5:q * W5 + W5 + N - 1], N)   # [W5][N]
        e = np.sum(np.abs(win) ** 2, axis=1)
        a = np.abs(win @ np.conj(p).T) ** 2                                                # [W5][3]
        C += np.where(e > 0, a.T / np.where(e > 0, e, 1.0), 0.0)
    return C


def metric(C):
    """-> (root, lag, peak, p2avg): the first maximum in (root, lag) order over the mean of its root"""
    i = int(np.argmax(C.reshape(-1)))     # numpy's argmax is the first maximum in C order
    r, n = divmod(i, C.shape[1])
    mean = float(np.mean(C[r]))
    return r, n, float(C[r, n]), (float(C[r, n]) / mean if mean > 0 else 0.0)


def decide(hyp, p2avg, peak, nof_periods=2, threshold=20.0, min_spacing_hz=1.4e6):
    """hyp: [(k, f_k)], p2avg and peak per hypothesis -> indices accepted, in the order of acceptance"""
    floor_peak = threshold * nof_periods / N
    cand = sorted((i for i in range(len(hyp)) if p2avg[i] >= threshold and peak[i] >= floor_peak), key=lambda i: (-p2avg[i], abs(hyp[i][1]), hyp[i][0]))
    acc = []
    for i in cand:
        if all(abs(hyp[i][1] - hyp[j][1]) >= min_spacing_hz for j in acc):
            acc.append(i)
    return acc


def scan(x, rate_in, nof_periods=2, threshold=20.0, min_spacing_hz=1.4e6, **kw):
    """x: one antenna of the head of a recording -> (hypotheses, [(root, lag, peak, p2avg)], accepted indices)"""
    hyp = hypotheses(rate_in, **kw)
    plan = ChannelPlan(rate_in)
    n = channel_samples(nof_periods)
    lo, hi = plan.span(0, n)
    assert len(x) >= hi, "the head is shorter than the scan reads"
    x = np.asarray(x)[:hi]
    met = []
    for k, f in hyp:
        y = plan.apply(mix(x, 0, tuning_word(f, rate_in)), 0, n)
        met.append(metric(correlate(y, nof_periods)))
    return hyp, met, decide(hyp, [m[3] for m in met], [m[2] for m in met], nof_periods, threshold, min_spacing_hz)


# ---- recordings ----
RATE_TWO = 7.68e6
# (scenario overrides, carrier in Hz, amplitude, up-sampling factor to 7.68 MS/s, lead in native samples)
TWO_CELLS = [(dict(nof_prb=6, cell_id=77, cp=1), 1.5e6, 1.0, 4, 700), (dict(nof_prb=15, cell_id=301, cp=0), -1.4e6, 10.0 ** -0.5, 2, 2500)]


NOISE_DB, NOISE_SEED = 20.0, 21


@functools.lru_cache(maxsize=None)
def two_cell_recording():
    """computed once per session, shared and left unchanged by the tests: a 7.68 MS/s recording of one antenna that holds a 6-block cell at +1.5 MHz and a 15-block
    cell at -1.4 MHz, 10 dB weaker.  Each is a lsn_testlib.sync_capture at its own rate (noise in front, then whole subframes from subframe 3 of a frame on),
    brought to 7.68 MS/s by resample_cases.fft_convert and moved to its carrier by ddc_cases.carrier; white noise 20 dB under the stronger cell's power fills the band.
    -> (x complex64 [n], [dict(f_hz, cell_id, cp, sf_idx, sf_start in samples of the 1.92 MS/s channel)])"""
    from ddc_cases import carrier
    from lsn_testlib import scenario, sync_capture
    from resample_cases import fft_convert
    parts, truth = [], []
    for over, f0, amp, up, lead in TWO_CELLS:
        sc = scenario("small", seed=5, start_tti=10 * 77 + 3, **over)
        x, _ = sync_capture(sc, lead, 3)
        nat = 1920 * 4 // up                                            # samples per subframe at the cell's own rate
        parts.append((fft_convert(x, up, 1), f0, amp))
        truth.append(dict(f_hz=f0, cell_id=over["cell_id"], cp=over["cp"], sf_idx=5, sf_start=(lead + 2 * nat) * up // 4))
    n = min(len(p[0]) for p in parts)
    # one receiver noise floor over the whole recorded band, NOISE_DB under the stronger cell's power: a recording made by a radio has one, the up-conversion
    # (which zero-pads the spectrum) leaves none
    rng = np.random.default_rng(NOISE_SEED)
    power = float(np.mean(np.abs(parts[0][2] * parts[0][0][:n]) ** 2))
    total = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * math.sqrt(0.5 * power * 10.0 ** (-NOISE_DB / 10.0))
    for y, f0, amp in parts:
        total += amp * y[:n] * carrier(n, f0, RATE_TWO)
    return total.astype(np.complex64), truth


@functools.lru_cache(maxsize=None)
def noise_recording(seed=3):
    """complex noise of the two-cell recording's length"""
    n = len(two_cell_recording()[0])
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def model_scan(which):
    """the model's scan of the two-cell ("cells") or the noise ("noise") recording, P = 2: computed once per session"""
    x = two_cell_recording()[0] if which == "cells" else noise_recording()
    return scan(x, RATE_TWO, nof_periods=2)

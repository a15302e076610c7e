"""Shared by the frequency-translation tests (CPU and GPU): the float64 model of the mixer in front of the resampler, written from DESIGN.md section 3.1b
("Frequency translation") and not from the kernel, offsets that keep shifted tones on the exact grid of resample_cases, and recordings that hold a cell off
their centre - one cell of an offset-tuned capture, or two cells side by side in a wideband capture.

Model: with W = floor(center_offset_hz / rate_in * 2^64 + 1/2) mod 2^64 (the quotient of the two doubles taken exactly), sample n of the recording is
multiplied by exp(-2 pi j (n W mod 2^64) / 2^64) - the phase reduced in Python integers, float64 exponential, no table - and handed to resample_model.Plan."""
import functools
import math
from fractions import Fraction

import numpy as np

from resample_cases import LEAD, Q, TAIL, fft_convert, tone
from resample_model import passband_hz

M64 = 2 ** 64


def tuning_word(center_offset_hz, rate_in):
    return int((2 * Fraction(float(center_offset_hz)) / Fraction(float(rate_in)) * M64 + 1) // 2) % M64


def mix(x, in_base, W):
    """x[0] = sample in_base of the recording (axis 0: samples) -> complex128, sample n times exp(-2 pi j (n W mod 2^64) / 2^64)"""
    x = np.asarray(x).astype(np.complex128)
    ph = np.array([((n * W) % M64) / M64 for n in range(int(in_base), int(in_base) + x.shape[0])], dtype=np.float64)
    return x * np.exp(-2j * np.pi * ph).reshape((-1,) + (1,) * (x.ndim - 1))


def model_resample(center_offset_hz, plan, x, in_base, n_out, m0=0, with_bound=False):
    """the float64 model of lsn_resample with center_offset_hz: mixer, then the plan's filter (|mix(x)| = |x|: the bound of Plan.apply is the mixed one's)"""
    return plan.apply(mix(x, in_base, tuning_word(center_offset_hz, plan.rate_in)), m0, n_out, in_base=in_base, with_bound=with_bound)


def offsets_k0(rate_in, nof_prb):
    """k0 of the offsets rate_in k0 / Q a pair is tested at: the largest the acceptance rule |f0| + B <= rate_in / 2 admits and a small one, both signs"""
    kmax = int(math.floor((0.5 * rate_in - passband_hz(nof_prb)) / rate_in * Q))
    assert kmax > 7
    return [kmax, -kmax, 7, -7]


def offset_hz(rate_in, k0):
    return rate_in * k0 / Q


def shifted(resample_fn, k0):
    """check_tones hands resample_fn the tone k (rate_in k / Q); the recording holds it at f0 + f: the tone times exp(+2 pi j k0 n / Q) with n the sample's
    index in the recording, exact in integers.  -> a resample_fn for check_tones that builds that recording and hands it to resample_fn(plan, x, in_base,
    n_out), which translates by -f0 and resamples: the tone must come out at f again"""
    def fn(plan, x, in_base, n_out):
        return resample_fn(plan, x * tone(k0, in_base, in_base + len(x)), in_base, n_out)
    return fn


# ---- recordings with a cell off their centre ----
def carrier(n, f0_hz, rate_hz):
    """exp(+2 pi j f0 n / rate) for n = 0 .. n - 1: f0 / rate = p / q in integers (the rates and offsets of CASES are whole Hz), phase (p n mod q) / q"""
    fr = Fraction(int(f0_hz), int(rate_hz))
    assert fr == Fraction(f0_hz) / Fraction(rate_hz)
    p, q = fr.numerator, fr.denominator
    return np.exp(2j * np.pi * ((p * np.arange(n, dtype=np.int64)) % q) / q)


def wideband(cells, num, den, native, channel_hz=None):
    """cells: [(iq[nsf][antenna][sflen] at the native rate, carrier in Hz relative to the recording's centre, amplitude)], all of the same shape.  Each capture goes
    through fft_convert to the file rate native * num / den and is continued periodically by LEAD samples in front and TAIL behind (as
    resample_cases.foreign_capture); then it is moved to its carrier - the phase counts samples of the FILE - and the cells are added.
    channel_hz (recordings of several cells): every capture is first confined to |f| <= channel_hz / 2, its own channel.  A capture of the synthetic transmitter
    fills its whole sampled band: receiver noise 30 dB under the signal out to +-15.36 MHz, and the side lobes of unfiltered CP-OFDM.  Added 19.8 MHz away, that
    is interference INSIDE the neighbour's occupied band (measured: -28 dB over its outer quarter, -40 dB elsewhere) which no translation or filter removes - a
    brick-wall FFT down-conversion of such a sum does not return the wanted cell's records either.  A recording of two carriers has one noise floor, and a base
    station's channel filter keeps its emissions in its channel (TS 36.104: 45 dB ACLR); the mask restores both.
    -> (rate_in, file samples [sample][antenna] complex128); sample LEAD of the file is the first sample of every capture"""
    rate_in = native * num / den
    assert rate_in == int(rate_in)
    f = None
    for iq, f0, amp in cells:
        x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, iq.shape[1])   # [sample][antenna]
        y = fft_convert(x, num, den)
        if channel_hz is not None:
            Y = np.fft.fft(y, axis=0)
            Y[np.abs(np.fft.fftfreq(len(y), 1.0 / rate_in)) > 0.5 * channel_hz] = 0.0
            y = np.fft.ifft(Y, axis=0)
        y = np.concatenate([y[len(y) - LEAD:], y, y[:TAIL]])
        y = amp * y * carrier(len(y), f0, rate_in)[:, None]
        f = y if f is None else f + y
    return rate_in, f


# name -> (file rate as (num, den) of the wanted cell's native rate, [(cell, carrier in Hz, amplitude)]); the FIRST cell is the one that is decoded.
# Cell "A" and the single cells are streams of srs_streams.STREAMS; "B" is A's scenario with another seed and cell_id (cell_b below).
CASES = {
    "two_cells_a": ((2, 1), [("A", 9.9e6, 1.0), ("B", -9.9e6, 1.0)]),
    "two_cells_b": ((2, 1), [("B", -9.9e6, 1.0), ("A", 9.9e6, 1.0)]),
    "prb50_plus_3p9": ((625, 384), [("prb50_1port_extcp", 3.9e6, 1.0)]),
    "prb25_plus_300k": ((1, 1), [("prb25_2port", 300e3, 1.0)]),
}
# Not a case: the two-cell recording with the unwanted cell 20 dB stronger (amplitude 10.0).  It does not pass the model round trip (cell B: 51 of its 66
# records) and DESIGN 3.1b says why: the filter's transition band hands the neighbour to the guard bins undamped, and the receiver's rectangular symbol
# window leaks about -40 dB of it into the occupied bins.
SPACING = 19.8e6   # contiguous 20 MHz carriers: the channel a cell of the two-cell recordings is confined to
CELL_A = "prb100_tm34_256qam"
CELL_B_SEED, CELL_B_ID = 10, 302


@functools.lru_cache(maxsize=None)
def cell(name):
    """computed once per session, shared and left unchanged by the tests -> (sc, tti0, iq at the 3GPP rate, oracle records, oracle trace, options) of "A", "B" or a stream of srs_streams.STREAMS"""
    import srs_streams as S
    from lsn_testlib import oracle_trace, scenario
    from parity import gen_subframes, oracle_records, run_oracle
    if name != "B":
        return S.stream(CELL_A if name == "A" else name)
    preset, nsf, over, opt = S.STREAMS[CELL_A]
    sc = scenario(preset, **dict(over, seed=CELL_B_SEED, cell_id=CELL_B_ID))
    tti0, iq, _ = gen_subframes(sc, nsf)
    _, _, orecs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
    return sc, tti0, iq, oracle_records(orecs), oracle_trace(), opt


@functools.lru_cache(maxsize=None)
def recording(case):
    """computed once per session, shared and left unchanged by the tests -> (sc, tti0, oracle records at the 3GPP rate, oracle trace, options, rate_in, native rate, center_offset_hz of the wanted cell,
    file samples [sample][antenna] complex128) - as resample_cases.foreign_capture, for the wanted (first) cell of the case"""
    from rate_convert import SYMBOL_SZ_3GPP
    how, cells = CASES[case]
    got = [cell(name) for name, _, _ in cells]
    sc, tti0, _, orecs, otrace, opt = got[0]
    native = 15000.0 * SYMBOL_SZ_3GPP[sc["nof_prb"]]
    rate_in, f = wideband([(g[2], f0, amp) for g, (_, f0, amp) in zip(got, cells)], how[0], how[1], native, channel_hz=SPACING if len(cells) > 1 else None)
    return sc, tti0, orecs, otrace, opt, rate_in, native, cells[0][1], f


def quantise(f, fmt):
    """file samples complex128 -> (array to write, sample_scale, the float64 values the product forms from it).  fmt 0: complex64.  fmt 1: int16 pairs, one
    LSB a power of two that puts the largest component of the recording between a quarter and half of full scale"""
    if fmt == 0:
        raw = f.astype(np.complex64)
        return raw, 0.0, raw.astype(np.complex128)
    peak = max(float(np.abs(f.real).max()), float(np.abs(f.imag).max()))
    scale = 2.0 ** math.ceil(math.log2(peak / 16384.0))
    raw = np.round(np.stack([f.real, f.imag], axis=-1) / scale).astype(np.int16)
    return raw, scale, (raw[..., 0] + 1j * raw[..., 1]) * scale

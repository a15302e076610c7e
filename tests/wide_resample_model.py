"""Float64 model of the resampler with the wide-ratio range, written from DESIGN.md section 3.1b ("accepted range") and 3.1o (the run geometry) - not from the
library.  The filter, the bank and the positions are resample_model.Plan's formulas restated here with the new range; the methods that only evaluate them
(position, span, max_out, phases, apply) are inherited.

Accepted: ratio = rate_in / rate_out <= 4 with Kaiser's estimate <= 192 (as before), or 4 < ratio <= 32 with rate_in <= 122.88e6, rate_out >= 3.84e6 and the
estimate <= 768.  Geometry of a plan with nominal step D (64.64): up to ratio 4 one lane per output, 512 outputs per run; above, G lanes per output - the
smallest power of two >= D, 8 .. 32 - and 4096 / G outputs per run; a run stages floor(run D) + T + 2 samples.

Also here: the 61.44 MS/s recording that holds a 100-PRB cell at -9.9 MHz and a 25-PRB cell (ratio 8) at +17 MHz."""
import functools
import math
from fractions import Fraction

import numpy as np

from resample_model import ATTEN_DB, PHASES, Plan, passband_hz

MAX_RATIO, MAX_TAPS = 4.0, 192
WIDE_MAX_RATIO, WIDE_MAX_RATE_IN, WIDE_MIN_RATE_OUT, WIDE_MAX_TAPS = 32.0, 122.88e6, 3.84e6, 768
SYMBOL_SZ = ({6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}, {6: 128, 15: 256, 25: 384, 50: 768, 75: 1024, 100: 1536})   # 3GPP, srsRAN


def kaiser_estimate(rate_in, rate_out, passband):
    width = (min(rate_in, rate_out) - 2.0 * passband) / rate_in
    return (ATTEN_DB - 7.95) / (14.36 * width) + 1.0 if width > 0 else math.inf


def accepted(rate_in, rate_out, passband):
    ratio, want = rate_in / rate_out, kaiser_estimate(rate_in, rate_out, passband)
    if ratio <= MAX_RATIO:
        return want <= MAX_TAPS
    return ratio <= WIDE_MAX_RATIO and rate_in <= WIDE_MAX_RATE_IN and rate_out >= WIDE_MIN_RATE_OUT and want <= WIDE_MAX_TAPS


def geometry(step, taps):
    """-> (lanes per output or 0, outputs per run, samples staged per run) of a plan with nominal step `step` (a Python integer, 64.64)"""
    if step <= 4 << 64:
        grp, run = 0, 512
    else:
        grp = 8
        while grp < 32 and (grp << 64) < step:
            grp *= 2
        run = 4096 // grp
    return grp, run, ((run * step) >> 64) + taps + 2


class WidePlan(Plan):
    def __init__(self, rate_in, rate_out, passband, first_sample=0, first_frac=0.0):
        rate_in, rate_out = float(rate_in), float(rate_out)
        if not accepted(rate_in, rate_out, passband):
            raise ValueError("outside the accepted range")
        self.rate_in, self.rate_out = rate_in, rate_out
        self.step = int((2 * Fraction(rate_in) / Fraction(rate_out) * 2 ** 64 + 1) // 2)
        self.start = (int(first_sample) << 64) + int(Fraction(first_frac) * 2 ** 64)
        self.rho = max(1.0, rate_in / rate_out)
        self.taps = T = max(4, 2 * int(math.ceil(kaiser_estimate(rate_in, rate_out, passband) / 2.0)))
        beta = 0.1102 * (ATTEN_DB - 8.7)
        t = np.arange(T)[None, :] - T / 2 + 1 - np.arange(PHASES + 1)[:, None] / PHASES
        u = np.clip(1.0 - (2.0 * t / T) ** 2, 0.0, None)
        self.H = np.sinc(t / self.rho) / self.rho * np.i0(beta * np.sqrt(u)) / np.i0(beta)
        self.H[np.abs(t) > T / 2] = 0.0
        self.grp, self.run, self.run_span = geometry(self.step, T)


# ---- recording (a): two cells of different bandwidth in a 61.44 MS/s recording, the narrow one at ratio 8 ----
WIDE_RATE = 61.44e6
# (stream, carrier, the channel the capture is confined to, file rate as (num, den) of the native rate)
WIDE_CELLS = (("prb100_tm34_256qam", -9.9e6, 19.8e6, (2, 1)), ("prb25_2port", 17e6, 5e6, (8, 1)))
WIDE_NSF = 12   # subframes of each cell inside the file: the 100-PRB stream's length


@functools.lru_cache(maxsize=None)
def wide_recording(strong_db=0.0):
    """computed once per session, shared and left unchanged by the tests -> ([(sc, tti0, oracle records of the first WIDE_NSF subframes, options, carrier in Hz,
    native rate)] per cell, file samples [sample][antenna] complex128); sample LEAD of the file is the first sample of both captures.  strong_db: the 100-PRB
    cell's level above the 25-PRB cell's"""
    from ddc_cases import carrier, cell
    from parity import oracle_records, run_oracle
    from resample_cases import LEAD, TAIL, fft_convert
    out, parts = [], []
    for name, f0, channel_hz, (num, den) in WIDE_CELLS:
        sc, tti0, iq, orecs, _, opt = cell(name)
        native = 15000.0 * SYMBOL_SZ[0][sc["nof_prb"]]
        assert native * num / den == WIDE_RATE and iq.shape[0] >= WIDE_NSF and iq.shape[1] == 2
        if iq.shape[0] > WIDE_NSF:
            iq = iq[:WIDE_NSF]
            _, _, recs = run_oracle(sc, tti0, iq, taps=False, **opt)
            orecs = oracle_records(recs)
        x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, iq.shape[1])   # [sample][antenna]
        y = fft_convert(x, num, den)
        Y = np.fft.fft(y, axis=0)
        Y[np.abs(np.fft.fftfreq(len(y), 1.0 / WIDE_RATE)) > 0.5 * channel_hz] = 0.0
        y = np.fft.ifft(Y, axis=0)
        y = np.concatenate([y[len(y) - LEAD:], y, y[:TAIL]])
        amp = 10.0 ** (strong_db / 20.0) if sc["nof_prb"] == 100 else 1.0
        parts.append(amp * y * carrier(len(y), f0, WIDE_RATE)[:, None])
        out.append((sc, tti0, orecs, opt, f0, native))
    assert len(parts[0]) == len(parts[1]) == LEAD + WIDE_NSF * 61440 + TAIL
    return out, parts[0] + parts[1]

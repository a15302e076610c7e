"""Shared by the multi-cell replay tests (CPU and GPU): a 30.72 MS/s recording that holds two cells of DIFFERENT bandwidth - the 75-PRB and the 25-PRB stream of
srs_streams.STREAMS, both with two receive antennas.  ddc_cases.wideband wants captures of equal shape, so each capture is brought from its own native rate to
the file rate (FFT conversion of the whole capture), confined to its own channel as wideband(channel_hz=...) does, continued periodically by LEAD samples in front
and TAIL behind, moved to its carrier with the integer phase of ddc_cases.carrier, and the two are added at equal amplitude.  The file is as long as the SHORTER
capture (75 PRB, 20 subframes); the longer one (25 PRB, 24 subframes) is cut off where the file ends, so its replay is limited by max_subframes."""
import functools

import numpy as np

from ddc_cases import carrier, cell
from resample_cases import LEAD, TAIL, fft_convert

MIXED_RATE = 30.72e6
# (stream, carrier relative to the recording's centre, channel the capture is confined to, file rate as (num, den) of the native rate)
MIXED = (("prb75_4port", -4.5e6, 15e6, (4, 3)), ("prb25_2port", 7.5e6, 5e6, (4, 1)))
MIXED_NSF = 20   # subframes of each cell that lie inside the file


@functools.lru_cache(maxsize=None)
def mixed_recording():
    """computed once per session, shared and left unchanged by the tests -> ([(sc, tti0, oracle records of the first MIXED_NSF subframes, options, carrier in Hz,
    native rate)] per cell, file samples [sample][antenna] complex128); sample LEAD of the file is the first sample of both captures"""
    from parity import oracle_records, run_oracle
    from rate_convert import SYMBOL_SZ_3GPP
    out, parts = [], []
    for name, f0, channel_hz, (num, den) in MIXED:
        sc, tti0, iq, orecs, _, opt = cell(name)
        native = 15000.0 * SYMBOL_SZ_3GPP[sc["nof_prb"]]
        assert native * num / den == MIXED_RATE and iq.shape[0] >= MIXED_NSF
        if iq.shape[0] > MIXED_NSF:
            _, _, recs = run_oracle(sc, tti0, iq[:MIXED_NSF], taps=False, **opt)
            orecs = oracle_records(recs)
        x = np.ascontiguousarray(iq.transpose(0, 2, 1)).reshape(-1, iq.shape[1])   # [sample][antenna]
        y = fft_convert(x, num, den)
        Y = np.fft.fft(y, axis=0)
        Y[np.abs(np.fft.fftfreq(len(y), 1.0 / MIXED_RATE)) > 0.5 * channel_hz] = 0.0
        y = np.fft.ifft(Y, axis=0)
        y = np.concatenate([y[len(y) - LEAD:], y, y[:TAIL]])
        parts.append(y * carrier(len(y), f0, MIXED_RATE)[:, None])
        out.append((sc, tti0, orecs, opt, f0, native))
    n = min(len(p) for p in parts)
    assert n == LEAD + MIXED_NSF * 30720 + TAIL
    return out, parts[0][:n] + parts[1][:n]

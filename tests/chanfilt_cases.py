"""Shared by the channel-filter tests (CPU and GPU): the recordings ddc_cases keeps out of its cases - two 100-PRB cells 9.9 MHz either side of the centre of a
61.44 MS/s file, the unwanted one 20 dB stronger - and the filter geometries the tests design."""
import functools

import numpy as np

from ddc_cases import SPACING, cell, quantise, wideband   # noqa: F401  (quantise: re-exported for the tests)
from resample_cases import Q, tone
from resample_model import passband_hz

RATE = 61.44e6
B100 = passband_hz(100)
STOP = SPACING - B100        # 10.785 MHz: the neighbour's nearest occupied edge
# (rate_in, pass band, stop band, L)
GEOMETRIES = [(RATE, B100, STOP, 88), (RATE, B100, B100 + 310e3, 498), (30.72e6, passband_hz(25), 3.0e6, 105), (RATE, B100, RATE / 2, 8)]

# name -> [(cell, carrier in Hz, amplitude)]; the FIRST cell is the one that is decoded, the other one is 20 dB stronger
CASES = {
    "b_wanted": [("B", -9.9e6, 1.0), ("A", 9.9e6, 10.0)],
    "a_wanted": [("A", 9.9e6, 1.0), ("B", -9.9e6, 10.0)],
}
NSF = 12


@functools.lru_cache(maxsize=None)
def recording(case):
    """computed once per session, shared and left unchanged by the tests -> as ddc_cases.recording: (sc, tti0, oracle records at the 3GPP rate, oracle trace,
    options, rate_in, native rate, center_offset_hz of the wanted cell, file samples [sample][antenna] complex128)"""
    from rate_convert import SYMBOL_SZ_3GPP
    cells = CASES[case]
    got = [cell(name) for name, _, _ in cells]
    sc, tti0, _, orecs, otrace, opt = got[0]
    native = 15000.0 * SYMBOL_SZ_3GPP[sc["nof_prb"]]
    rate_in, f = wideband([(g[2], f0, amp) for g, (_, f0, amp) in zip(got, cells)], 2, 1, native, channel_hz=SPACING)
    assert rate_in == RATE
    return sc, tti0, orecs, otrace, opt, rate_in, native, cells[0][1], f


def check_filter_tones(fn, m, k0, base):
    """fn(x, in_base, n0, n) -> y1[n0 .. n0 + n - 1] of a recording x that holds tones at f0 + f, f0 = rate k0 / Q.  -> (worst pass-band error, relative RMS;
    largest stop-band gain) over exact tones on the grid rate k / Q: |f| <= B with the edges, |f| >= S from the first grid point at or behind S on"""
    R, L, n = m.rate_in, m.L, 3000
    n0 = base + L if base else 0                       # base 0: the first L outputs read the zeros in front of the recording and are not a tone's
    lo, hi = max(n0 - L, 0), n0 + n + L
    skip = L if n0 == 0 else 0
    kb = int(np.floor(m.passband / R * Q))
    ks = int(np.ceil(m.stopband / R * Q))
    worst_pass = worst_stop = 0.0
    for k in sorted({-kb, -kb // 2, -3, 0, 1, kb // 3, kb - 1, kb}):
        y = fn(tone(k + k0, lo, hi), lo, n0, n)
        ref = tone(k, n0, n0 + n)
        worst_pass = max(worst_pass, float(np.sqrt(np.sum(np.abs(y[skip:] - ref[skip:]) ** 2) / np.sum(np.abs(ref[skip:]) ** 2))))
    stop = sorted({s * k for s in (-1, 1) for k in list(range(ks, Q // 2 + 1, 61)) + [ks, ks + 1, ks + 2, Q // 2]})
    for k in stop:
        y = fn(tone(k + k0, lo, hi), lo, n0, n)
        worst_stop = max(worst_stop, float(np.sqrt(np.mean(np.abs(y[skip:]) ** 2))))
    return worst_pass, worst_stop


# (geometry, k0 of the offsets the tones are tested at): 660 is 9.9 MHz at 61.44 MS/s, 400 is 3.0 MHz at 30.72 MS/s
TONE_CASES = [(GEOMETRIES[0], (660, -660, 0)), (GEOMETRIES[1], (660, -660)), (GEOMETRIES[2], (400, -400, 0))]

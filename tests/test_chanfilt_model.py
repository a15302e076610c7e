"""The channel filter in front of the resampler, without a GPU: the library's design, refusals and spans against the float64 model of
tests/chanfilt_model.py, the model's selectivity on exact tones, and the round trip of the recordings with a neighbour 20 dB stronger through the model and the
CPU oracle - with the filter every record comes back, without it they do not.  The GPU tests (test_gpu_chanfilt.py) hold the kernel to this model and replay
the same recordings."""
import ctypes as C

import numpy as np
import pytest

import ltesniffer_amd as la
from chanfilt_cases import B100, GEOMETRIES, NSF, RATE, STOP, TONE_CASES, check_filter_tones, quantise, recording
from chanfilt_model import Design, two_stage
from ddc_cases import model_resample
from resample_cases import FAR, LEAD, Q
from resample_model import Plan, passband_hz
from srs_streams import edge_blocks, failed_records

INVALID = -2   # LSN_ERROR_INVALID_INPUTS


@pytest.mark.parametrize("rate,B,S,L", GEOMETRIES)
def test_design_is_the_models(rate, B, S, L):
    m = Design(rate, B, S)
    d = la.channel_filter_design(rate, B, S)
    assert m.L == L and d["L"] == L and len(d["taps"]) == 2 * L + 1 and d["fc"] == m.fc
    ulp = np.spacing(np.abs(m.g32))
    assert np.all(np.abs(d["taps"].astype(np.float64) - m.g) <= ulp), float(np.max(np.abs(d["taps"].astype(np.float64) - m.g) / ulp))
    assert np.array_equal(d["taps"], d["taps"][::-1]) and abs(float(np.sum(m.g)) - 1.0) < 1e-3


def _design_rc(rate, B, S, size=None):
    d = la.ChannelFilterDesign(C.sizeof(la.ChannelFilterDesign) if size is None else size, 0, 0, 0, 0.0)
    return la.lib().lsn_channel_filter_design(rate, B, S, C.byref(d), None, 0), d


def _span(cfg, n_out=1000, in_end=10 ** 6):
    sp = la.ResampleSpan()
    rc = la.lib().lsn_channel_filter_span(C.byref(cfg), n_out, in_end, C.byref(sp))
    return rc, (sp.in_lo, sp.in_hi, sp.max_out, sp.taps)


def test_refusals_and_struct_sizes():
    assert C.sizeof(la.ChannelFilterDesign) == 24 and C.sizeof(la.ChannelFilterCfg) == 64
    assert _design_rc(RATE, B100, STOP)[0] == 0
    edge = B100 + 0.0049 * RATE                    # L = 512 needs S - B >= (80 - 7.95) / (14.36 * 1024) R = 0.0048998 R
    assert _design_rc(RATE, B100, edge)[0] == 0 and _design_rc(RATE, B100, edge)[1].half_len == 512
    for S in (B100, B100 - 1.0, 0.0, -1e6, RATE / 2 + 1.0, 1e30, float("nan"), float("inf"), float("-inf"), B100 + 300e3):
        assert _design_rc(RATE, B100, S)[0] == INVALID, S
        with pytest.raises(ValueError):
            Design(RATE, B100, S)
    for rate, B in ((0.0, B100), (float("nan"), B100), (RATE, 0.0), (RATE, float("nan"))):
        assert _design_rc(rate, B, STOP)[0] == INVALID
    for size in (0, 16, 23, 25, 32):
        assert _design_rc(RATE, B100, STOP, size)[0] == INVALID, size
    taps = np.zeros(177, dtype=np.float32)
    d = la.ChannelFilterDesign(24, 0, 0, 0, 0.0)
    assert la.lib().lsn_channel_filter_design(RATE, B100, STOP, C.byref(d), taps.ctypes.data, 176) == INVALID      # the taps do not fit
    assert la.lib().lsn_channel_filter_design(RATE, B100, STOP, C.byref(d), taps.ctypes.data, 177) == 0 and taps[88] > 0.3
    good = la._channel_filter_cfg(1, RATE, B100, STOP, 9.9e6, 0, 0, la.FILE_CF32, 0.0)
    assert _span(good)[0] == 0
    for size in (0, 56, 63, 65, 72, 128):
        bad = la._channel_filter_cfg(1, RATE, B100, STOP, 9.9e6, 0, 0, la.FILE_CF32, 0.0)
        bad.struct_size = size
        assert _span(bad)[0] == INVALID, size
    # the cell lies inside the recording: the resampler's rule, applied by stage 1 because stage 2 no longer sees the offset
    cedge = RATE / 2 - B100
    for f0, want in ((cedge, 0), (-cedge, 0), (cedge + 1.0, INVALID), (float("nan"), INVALID), (float("inf"), INVALID)):
        assert _span(la._channel_filter_cfg(1, RATE, B100, STOP, f0, 0, 0, la.FILE_CF32, 0.0))[0] == want, f0
    for kw in (dict(nof_antennas=0), dict(nof_antennas=9), dict(sample_format=3)):
        args = dict(nof_antennas=1, sample_format=la.FILE_CF32)
        args.update(kw)
        assert _span(la._channel_filter_cfg(args["nof_antennas"], RATE, B100, STOP, 0.0, 0, 0, args["sample_format"], 0.0))[0] == INVALID


@pytest.mark.parametrize("rate,B,S,L", GEOMETRIES)
def test_spans_widen_by_exactly_L(rate, B, S, L):
    m = Design(rate, B, S)
    for out_first, n_out, in_end in ((0, 1000, 10 ** 6), (12345, 1, 20000), (FAR, 4096, FAR + 5000), (0, 0, L), (7, 10, L + 7)):
        sp = la.channel_filter_span(n_out, in_end, rate, B, S, out_first=out_first)
        lo, hi = m.span(out_first, n_out)
        assert (sp["in_lo"], sp["in_hi"]) == (out_first - L, out_first + n_out + L) == (lo, hi)
        assert sp["max_out"] == max(m.max_out(in_end) - out_first, 0) == max(in_end - L - out_first, 0) and sp["taps"] == 2 * L + 1
    # stage 2 reading [lo, hi) makes the two stages read [lo - L, hi + L), and the recording carries L fewer samples for stage 2
    plan = Plan(rate, 15000.0 * {B100: 2048}.get(B, 512), B, 1000, 0.25)
    r = la.resample_span(5000, 10 ** 6 - L, rate, plan.rate_out, 1000, 0.25, passband_hz=B)
    lo, hi = plan.span(0, 5000)
    assert (r["in_lo"], r["in_hi"]) == (lo, hi) and r["max_out"] == plan.max_out(10 ** 6 - L)
    sp = la.channel_filter_span(hi - lo, 10 ** 6, rate, B, S, out_first=lo)
    assert (sp["in_lo"], sp["in_hi"]) == (lo - L, hi + L)


def test_cells_stopbands():
    assert la.cells_stopbands([9.9e6, -9.9e6], [100, 100], RATE) == [STOP, STOP] == [10.785e6, 10.785e6]
    assert la.cells_stopbands([9.9e6], [100], RATE) == [0.0]
    # the nearest neighbour decides; a far one is capped at rate / 2; one that overlaps gives no filter
    s = la.cells_stopbands([0.0, 15e6, -25e6], [25, 50, 25], RATE)
    assert s == [15e6 - passband_hz(50), 15e6 - passband_hz(25), 25e6 - passband_hz(25)]
    assert la.cells_stopbands([-20e6, 20e6], [25, 25], RATE) == [RATE / 2, RATE / 2]
    assert la.cells_stopbands([0.0, 5e6], [100, 100], RATE) == [0.0, 0.0]
    with pytest.raises(ValueError):
        la.cells_stopbands([0.0, 18.03e6 + 200e3], [100, 100], RATE)      # 200 kHz between the occupied edges: L would exceed 512
    with pytest.raises(ValueError):
        la.cells_stopbands([0.0, float("nan")], [100, 100], RATE)
    with pytest.raises(ValueError):
        la.cells_stopbands([], [], RATE)


@pytest.mark.parametrize("base", [0, FAR])
@pytest.mark.parametrize("geometry,k0s", TONE_CASES)
def test_model_meets_the_selectivity_requirement(geometry, k0s, base):
    """tones at f0 + f, |f| <= B, come out at f within -60 dB relative RMS (the resampler's requirement); tones at |f| >= S - S itself included - come out at
    least 77 dB down (the design reaches 79.9 dB in the geometries tried; 3 dB are left for those not tried)"""
    rate, B, S, L = geometry
    m = Design(rate, B, S)
    h_pass = np.abs(m.response(np.linspace(-B, B, 401)) - 1.0).max()
    h_stop = np.abs(m.response(np.concatenate([[S, -S], np.linspace(S, rate / 2, 2001)]))).max()
    print("channel filter L = %d: response of the float32 taps: pass band %.1f dB, stop band %.1f dB" % (L, 20 * np.log10(h_pass), 20 * np.log10(h_stop)))
    assert h_pass <= 1e-3 and h_stop <= 10 ** (-77 / 20)
    for k0 in k0s:
        f0 = rate * k0 / Q
        worst_pass, worst_stop = check_filter_tones(lambda x, in_base, n0, n: m.apply(x, in_base, n0, n, f0), m, k0, base)
        print("channel filter model L = %d, offset %+.1f kHz, base %d: pass band %.1f dB, stop band %.1f dB" %
              (L, f0 / 1e3, base, 20 * np.log10(worst_pass), 20 * np.log10(worst_stop)))
        assert worst_pass <= 1e-3 and worst_stop <= 10 ** (-77 / 20), (k0, worst_pass, worst_stop)


ROUND_TRIPS = [("b_wanted", la.FILE_CF32), ("a_wanted", la.FILE_CF32), ("b_wanted", la.FILE_SC16)]


@pytest.mark.parametrize("case,fmt", ROUND_TRIPS)
def test_round_trip_through_the_oracle_needs_the_filter(case, fmt):
    """recording with the neighbour 20 dB stronger -> file format -> model stage 1 (mixer + channel filter) -> resample_model.Plan -> complex64 -> oracle: every
    record of the oracle's run on the wanted cell's original capture, byte for byte, no code block at the edge.  Control: the same recording through the
    mixer and the resampler alone does NOT return all records - the filter is what passes it."""
    from lsn_testlib import oracle_trace
    from parity import oracle_records, run_oracle
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording(case)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    _, _, x = quantise(f, fmt)
    nant, sflen = f.shape[1], int(native) // 1000
    m = Design(rate_in, B100, STOP)
    plan = Plan(rate_in, native, B100, LEAD, 0.0)
    assert m.L == 88 and plan.max_out(m.max_out(len(f))) // sflen >= NSF

    def decode(y):
        iq = np.ascontiguousarray(y.reshape(NSF, sflen, nant).transpose(0, 2, 1)).astype(np.complex64)
        _, _, recs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
        return oracle_records(recs), oracle_trace()

    recs, trace = decode(two_stage(m, plan, x, f0, NSF * sflen))
    assert edge_blocks(trace) == [] and failed_records(recs) == []
    assert recs == orecs, "records differ: %d vs %d" % (len(recs), len(orecs))
    plain, _ = decode(model_resample(f0, plan, x, 0, NSF * sflen))
    same = sum(1 for r in plain if r in orecs)
    print("%s fmt %d: with the filter %d of %d records; without it %d records, %d of them the oracle's" % (case, fmt, len(recs), len(orecs), len(plain), same))
    assert plain != orecs

"""Carrier scan without a GPU: lsn_carrier_scan_plan and lsn_carrier_scan_decide against the float64 model of tests/scan_model.py (written from DESIGN.md section
3.1d), the model's decision on a recording of two cells and on noise, and lsn_resample's refusals, which the lifted caps of the scan's channel must not move."""
import ctypes as C

import numpy as np
import pytest

import ltesniffer_amd as la
import scan_model as M
from ddc_cases import tuning_word
from resample_model import passband_hz

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
RATES = [(7.68e6, 50), (25e6, None), (61.44e6, 382), (122.88e6, 764)]


@pytest.mark.parametrize("rate_in,taps", RATES)
def test_plan_equals_the_models_hypotheses_and_taps(rate_in, taps):
    """hypotheses (k, f_k bit for bit, tuning word), the number of taps by the formula (50 / 382 / 764), the bank within one float32 rounding of the model's H
    and dH, and the input the scan reads"""
    for kw in (dict(), dict(raster_hz=30e3, raster_offset_hz=7e3, nof_periods=1), dict(f_lo_hz=-1.05e6, f_hi_hz=2e6, nof_periods=3)):
        d = la.carrier_scan_plan(rate_in, with_bank=True, **kw)
        mk = {k: v for k, v in kw.items() if k != "nof_periods"}
        hyp = M.hypotheses(rate_in, **mk)
        plan = M.ChannelPlan(rate_in)
        P = kw.get("nof_periods", 2)
        assert d["nof_hypotheses"] == len(hyp) and d["k"] == [k for k, _ in hyp]
        assert np.array_equal(np.array(d["f_hz"]).view(np.uint64), np.array([f for _, f in hyp]).view(np.uint64))
        assert d["tuning_word"] == [tuning_word(f, rate_in) for _, f in hyp]
        assert d["taps"] == plan.taps and (taps is None or plan.taps == taps)
        assert d["nof_periods"] == P and d["nof_channel_samples"] == M.channel_samples(P) == (P + 1) * 9600 + 128
        assert d["nof_input_samples"] == plan.span(0, M.channel_samples(P))[1]
        H = plan.H
        scale = float(np.abs(H).max())
        assert np.abs(d["bank"][:, :, 0] - H[:512]).max() <= 2.0 ** -24 * scale
        assert np.abs(d["bank"][:, :, 1] - (H[1:] - H[:512])).max() <= 2.0 ** -23 * scale   # (the difference of two values rounded once)
    n = len(M.hypotheses(rate_in))
    edge = rate_in / 2 - M.B6
    assert n == 2 * int(np.floor(edge / 100e3)) + 1


def test_plan_refusals():
    L = la.lib()
    pl = la.CarrierScanPlan()

    def rc(cfg):
        return L.lsn_carrier_scan_plan(C.byref(cfg), C.byref(pl), None, 0, None)

    assert rc(la.carrier_scan_cfg(7.68e6)) == 0
    for rate in (1.92e6 - 1.0, 122.88e6 + 1.0, 0.0, -7.68e6, float("nan"), float("inf")):
        assert rc(la.carrier_scan_cfg(rate)) == INVALID, rate
    assert rc(la.carrier_scan_cfg(1.92e6)) == 0 and rc(la.carrier_scan_cfg(122.88e6)) == 0
    assert rc(la.carrier_scan_cfg(61.44e6, raster_hz=10e3)) == 0 and pl.nof_hypotheses == 6033
    assert rc(la.carrier_scan_cfg(61.44e6, raster_hz=7.36e3)) == INVALID      # 8197 hypotheses
    assert rc(la.carrier_scan_cfg(61.44e6, raster_hz=7.37e3)) == 0 and pl.nof_hypotheses <= 8192
    assert rc(la.carrier_scan_cfg(61.44e6, raster_hz=1e-3)) == INVALID
    assert rc(la.carrier_scan_cfg(7.68e6, f_lo_hz=10e3, f_hi_hz=90e3)) == INVALID  # none
    assert rc(la.carrier_scan_cfg(7.68e6, f_lo_hz=2e6, f_hi_hz=1e6)) == INVALID
    assert rc(la.carrier_scan_cfg(7.68e6, nof_periods=17)) == INVALID
    assert rc(la.carrier_scan_cfg(7.68e6, raster_hz=-100e3)) == INVALID
    for size in (0, C.sizeof(la.CarrierScanCfg) - 8, C.sizeof(la.CarrierScanCfg) + 8):
        cfg = la.carrier_scan_cfg(7.68e6)
        cfg.struct_size = size
        assert rc(cfg) == INVALID, size
    hyp = (la.CarrierMetric * 10)()
    assert L.lsn_carrier_scan_plan(C.byref(la.carrier_scan_cfg(7.68e6)), C.byref(pl), hyp, 10, None) == INVALID   # 65 do not fit
    with pytest.raises(ValueError):
        la.carrier_scan_plan(200e6)
    with pytest.raises(ValueError):
        M.hypotheses(61.44e6, raster_hz=7.36e3)
    with pytest.raises(ValueError):
        M.ChannelPlan(1.0e6)
    # the channel of lsn_carrier_channel: the same range, and the acceptance rule of center_offset_hz
    sp = la.ResampleSpan()
    for rate, f0, want in ((7.68e6, 3.285e6, 0), (7.68e6, 3.285e6 + 1.0, INVALID), (1.0e6, 0.0, INVALID), (130e6, 0.0, INVALID), (7.68e6, float("nan"), INVALID)):
        cfg = la._channel_cfg(1, rate, f0, 0, 0.0, 0, 0, la.FILE_CF32, 0.0)
        assert L.lsn_carrier_channel_span(C.byref(cfg), 100, 10 ** 6, C.byref(sp)) == want, (rate, f0)
    cfg = la._channel_cfg(1, 7.68e6, 0.0, 0, 0.0, 0, 0, la.FILE_CF32, 0.0)
    cfg.struct_size -= 8
    assert L.lsn_carrier_channel_span(C.byref(cfg), 100, 10 ** 6, C.byref(sp)) == INVALID


def test_model_finds_the_two_cells_and_suppresses_their_ghosts():
    """the 7.68 MS/s recording of a 6-block cell at +1.5 MHz and a 15-block cell at -1.4 MHz, 10 dB weaker: the model returns exactly those two offsets; the
    hypotheses 300 kHz beside the stronger carrier - 20 sub-carriers off: a time-shifted PSS through the part of the filter that still overlaps - are above the
    threshold before the suppression and gone after it"""
    x, truth = M.two_cell_recording()
    hyp, met, acc = M.model_scan("cells")
    f = [h[1] for h in hyp]
    p2 = {h[0]: m[3] for h, m in zip(hyp, met)}
    print("p2avg per k:", " ".join("%d:%.1f" % (k, v) for k, v in sorted(p2.items())))
    assert [f[i] for i in acc] == [1.5e6, -1.4e6], [(f[i], met[i]) for i in acc]
    assert sorted(f[i] for i in acc) == sorted(t["f_hz"] for t in truth)
    ghosts = [k for k in (12, 18, -17, -11) if p2[k] >= 20.0]
    assert ghosts and (12 in ghosts or 18 in ghosts), p2
    assert not any(hyp[i][0] in ghosts for i in acc)
    # finding 2 of DESIGN 3.1d: hypotheses 1.1 .. 1.4 MHz beside the strong carrier hold it only in the filter's transition band; their p2avg is large on a peak
    # that is none, one of them exactly min_spacing_hz away.  The floor on the peak (threshold P / N = 0.3125) is what keeps them out
    peak = {h[0]: m[2] for h, m in zip(hyp, met)}
    false = [k for k in p2 if p2[k] >= 20.0 and peak[k] < 20.0 * 2 / 128]
    print("p2avg >= 20 on a peak under the floor:", [(k, round(p2[k], 1), round(peak[k], 3)) for k in false])
    assert any(min(abs(k * 1e5 - 1.5e6), abs(k * 1e5 + 1.4e6)) >= 1.4e6 for k in false), false       # (not one the spacing rule would have dropped)
    assert all(peak[k] >= 20.0 * 2 / 128 for k in ghosts)
    # the product's decision on the model's metrics: the same answer
    got = la.carrier_scan_decide([(h[0], h[1], np.float32(m[3]), np.float32(m[2])) for h, m in zip(hyp, met)], M.RATE_TWO)
    assert got == acc


def test_decision_order_ties_and_spacing():
    hyp = [(k, k * 1e5) for k in range(-30, 31)]
    p2 = [0.0] * len(hyp)
    at = {k: i for i, (k, _) in enumerate(hyp)}
    for k, v in ((8, 50.0), (-8, 50.0), (-12, 50.0), (22, 49.0), (12, 30.0), (-30, 19.999), (30, 20.0), (0, 60.0)):
        p2[at[k]] = v
    peak = [1.0] * len(hyp)
    peak[at[0]] = 0.3124        # the largest metric, on a peak under the floor of 20 * 2 / 128 = 0.3125
    peak[at[22]] = 0.3125
    want = M.decide(hyp, p2, peak)
    # 0 is out (its peak); -8 before 8 (same metric, same |f|: the lower k), then -12 (same metric, larger |f|) is 400 kHz from -8: dropped; 22 is exactly 1.4 MHz
    # from 8: kept (only strictly closer is dropped); 12 and 30 are dropped; -30 is under the threshold
    assert [hyp[i][0] for i in want] == [-8, 8, 22]
    rows = [(k, f, v, pk) for (k, f), v, pk in zip(hyp, p2, peak)]
    assert la.carrier_scan_decide(rows, 7.68e6) == want
    assert la.carrier_scan_decide(rows, 7.68e6, min_spacing_hz=1.0) == M.decide(hyp, p2, peak, min_spacing_hz=1.0)
    assert [hyp[i][0] for i in M.decide(hyp, p2, peak, threshold=19.0, min_spacing_hz=1.0)] == [0, -8, 8, -12, 22, 12, 30, -30]
    assert la.carrier_scan_decide(rows, 7.68e6, threshold=19.0, min_spacing_hz=1.0) == M.decide(hyp, p2, peak, threshold=19.0, min_spacing_hz=1.0)
    assert [hyp[i][0] for i in M.decide(hyp, p2, peak, nof_periods=3)] == [-8, 8, 30]      # the floor follows P: 0.46875 takes 22 out, which had kept 30 out
    assert la.carrier_scan_decide(rows, 7.68e6, nof_periods=3) == M.decide(hyp, p2, peak, nof_periods=3)


def test_model_finds_nothing_in_noise():
    """complex noise of the recording's length, P = 2: no hypothesis reaches the threshold (about 1e-9 per scan)"""
    hyp, met, acc = M.model_scan("noise")
    worst = max(m[3] for m in met)
    assert acc == [] and worst < 20.0, "largest p2avg of the seeded noise: %.2f" % worst


def test_resample_refusals_are_where_they_were():
    """lsn_resample's own caps: ratio above 4 and more than 192 taps are refused as before, whatever the scan's channel is allowed"""
    L = la.lib()
    sp = la.ResampleSpan()

    def rc(rate_in, rate_out, B):
        cfg = la._resample_cfg(1, rate_in, rate_out, 0, 0.0, 0, 0, B, la.FILE_CF32, 0.0)
        return L.lsn_resample_span(C.byref(cfg), 100, 10 ** 6, C.byref(sp))

    assert rc(7.68e6, 1.92e6, M.B6) == 0 and sp.taps == 50                      # ratio 4: the resampler's own filter is the scan's at this rate
    assert rc(7.68e6 + 1.0, 1.92e6, M.B6) == INVALID                            # ratio above 4
    assert rc(61.44e6, 1.92e6, M.B6) == INVALID and rc(122.88e6, 1.92e6, M.B6) == INVALID
    assert rc(61.44e6, 30.72e6, passband_hz(100)) == 0
    # taps: (80 - 7.95) / (14.36 width) + 1 <= 192 <=> width >= 0.026269...; 30.72 -> 30.72 MS/s with B = 14.95e6: width 0.02669 passes, 14.97e6: 0.02539 does not
    assert rc(30.72e6, 30.72e6, 14.95e6) == 0 and sp.taps <= 192
    assert rc(30.72e6, 30.72e6, 14.97e6) == INVALID
    assert la.carrier_scan_plan(61.44e6)["taps"] == 382

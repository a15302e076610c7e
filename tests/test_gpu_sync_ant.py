"""The cell search and the carrier scan over all receive antennas on the GPU (k_pss_corr_ant, lsn_cell_search_ant, LSN_SCAN_ALL_ANTENNAS):
with one antenna every number is the one-antenna search's; with two the correlation lies inside the float32 bound of the float64 model (tests/sync_ant_model.py)
and the decisions are the model's on a cell whose channels are opposite, a cell absent from antenna 0 (which the search of antenna 0 misses) and a cell whose SSS
neither antenna decides alone; the scan finds two carriers of which each antenna holds only one."""
import os

import numpy as np
import pytest

import ltesniffer_amd as la
import sync_ant_cases as K
import sync_ant_model as M

pytestmark = pytest.mark.gpu
FIELDS = ("found", "cell_id", "n_id_2", "n_id_1", "sf_idx", "pss_pos", "sf_start", "cp")
FLOATS = ("pss_peak", "pss_p2avg", "sss_metric", "sss_second", "cfo_hz", "cfo_coarse_hz")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(g, o):
    assert [getattr(g, f) for f in FIELDS] == [getattr(o, f) for f in FIELDS], ([getattr(g, f) for f in FIELDS], [getattr(o, f) for f in FIELDS])
    a, b = [getattr(g, f) for f in FLOATS], [getattr(o, f) for f in FLOATS]
    assert np.array_equal(bits(a), bits(b)), (a, b)


@pytest.mark.parametrize("nof_prb,periods,force,on_device", [(6, 2, -1, False), (6, 2, 2, False), (25, 1, -1, False), (6, 2, -1, True)])
def test_one_antenna_is_the_one_antenna_search(nof_prb, periods, force, on_device):
    x = K.clean_cell(nof_prb=nof_prb, periods=periods)
    arg, arg2 = x, x[None, :]
    if on_device:
        import torch
        arg = torch.from_numpy(np.array(x).view(np.float32)).to("cuda:0").view(torch.complex64)
        arg2 = arg[None, :]
    kw = dict(nof_periods=periods, force_n_id_2=force, with_corr=True)
    r1, s1, c1 = la.cell_search(arg, nof_prb, **kw)
    r2, s2, per, c2 = la.cell_search_ant(arg2, nof_prb, **kw)
    assert r1 == r2 == 1 and s1.cell_id == 77
    same(s2, s1)
    assert np.array_equal(bits(c1), bits(c2)) and float(c2.max()) == s2.pss_peak
    p = per[0]
    assert np.array_equal(bits([p.pss_peak, p.sss_metric, p.sss_second, p.cfo_hz]), bits([s1.pss_peak, s1.sss_metric, s1.sss_second, s1.cfo_hz])) and p.n_id_1 == s1.n_id_1


@pytest.mark.parametrize("nof_prb,periods", [(6, 1), (6, 3), (25, 1), (25, 3)])
def test_correlation_of_two_antennas_against_the_model_within_the_float32_bound(nof_prb, periods):
    N = M.SYMBOL[nof_prb]
    x = K.two_antennas((1.0, -1.0), K.SNR_DB, 7, nof_prb=nof_prb, periods=3)
    rc, s, per, corr = la.cell_search_ant(x, nof_prb, nof_periods=periods, with_corr=True)
    rc2, s2, per2, corr2 = la.cell_search_ant(x, nof_prb, nof_periods=periods, with_corr=True)
    assert np.array_equal(bits(corr), bits(corr2)) and bytes(s) == bytes(s2) and [bytes(p) for p in per] == [bytes(p) for p in per2]
    reps = [M.MM.replica(r, N) for r in range(3)]
    need = (periods + 1) * 75 * N + N
    C, B, own = M.correlation(x[:, :need], reps, N, periods, with_bound=True)
    err = np.abs(corr.astype(np.float64) - C)
    worst = float(np.max(err / np.maximum(B, 1e-300)))
    print("k_pss_corr_ant N = %d, P = %d, A = 2: largest error / bound = %.3f (largest error %.3g, peak %.3f)" % (N, periods, worst, float(err.max()), float(C.max())))
    assert np.all(err <= B), worst
    assert rc == 1 and float(C.max()) > 0.1 * periods     # (the comparison is not one of zeros: a cell's peak, 0.38 per period at N = 512)
    # the antennas' own values at the common lag add up to the peak
    ri = s.n_id_2
    for a in range(2):
        assert abs(per[a].pss_peak - own[a][ri, s.pss_pos]) <= B[ri, s.pss_pos]
    assert abs(per[0].pss_peak + per[1].pss_peak - s.pss_peak) <= (2 * periods + 2) * M.U * s.pss_peak     # (another order of the same 2 P terms)


def _against_model(x, P=2):
    rc, s, per = la.cell_search_ant(x, K.NOF_PRB, nof_periods=P)
    m = M.search(x, K.NOF_PRB, P)
    assert rc == int(m["found"])
    for f in FIELDS:
        assert getattr(s, f) == int(m[f]), (f, getattr(s, f), m[f])
    for f in ("pss_peak", "pss_p2avg", "sss_metric", "sss_second"):
        assert abs(getattr(s, f) - m[f]) <= 1e-3 * abs(m[f]), (f, getattr(s, f), m[f])
    print("cfo_hz %.4f, model %.4f +- %.4f" % (s.cfo_hz, m["cfo_hz"], m["cfo_bound"]))
    assert abs(s.cfo_hz - m["cfo_hz"]) <= m["cfo_bound"]
    assert abs(s.cfo_coarse_hz - m["cfo_coarse_hz"]) <= 1.0
    for p, q in zip(per, m["per_ant"]):
        assert p.occurrence == q["occurrence"] and (p.n_id_1 == q["n_id_1"] or q["sss_metric"] < 1.01 * q["sss_second"]), (p.n_id_1, p.occurrence, q)
        assert abs(p.pss_peak - q["pss_peak"]) <= 1e-3 * max(q["pss_peak"], 1e-3) and abs(p.sss_metric - q["sss_metric"]) <= 1e-3 * q["sss_metric"]
    return s, per, m


def test_opposite_channels():
    """+1 and -1: the sum of the antennas holds no cell (asserted on the CPU and here), the combination finds it"""
    x = K.opposite()
    s, per, m = _against_model(x)
    assert s.found and s.cell_id == 77 and s.cp == 0 and (s.sf_start, s.sf_idx) == K.timing()
    rc, summed = la.cell_search((x[0] + x[1]).astype(np.complex64), K.NOF_PRB, nof_periods=2)
    assert rc == 0 and summed.pss_p2avg < 20.0


def test_cell_absent_from_antenna_0():
    """what the feature is for: the one-antenna search of antenna 0 misses the cell, the search over both antennas finds it and names antenna 1"""
    x = K.faded()
    rc0, s0 = la.cell_search(x[0], K.NOF_PRB, nof_periods=2)
    assert rc0 == 0 and not s0.found, s0.pss_p2avg
    s, per, m = _against_model(x)
    assert s.found and s.cell_id == 77 and (s.sf_start, s.sf_idx) == K.timing()
    assert per[1].pss_peak > 10.0 * per[0].pss_peak and per[1].n_id_1 == s.n_id_1


def test_sss_decision_that_neither_antenna_takes_alone():
    x = K.sss_case(*K.SSS_CASE)
    s, per, m = _against_model(x)
    assert s.found and s.cell_id == 77 and s.cp == 0 and (s.sf_start, s.sf_idx) == K.timing()
    assert s.sss_metric >= 1.2 * s.sss_second
    for p in per:
        assert p.n_id_1 != s.n_id_1 or p.sss_metric < 1.2 * p.sss_second


def test_strided_input_is_read_in_place():
    import torch
    x = K.opposite()
    n = x.shape[1]
    wide = np.zeros((2, n + 1000), dtype=np.complex64)
    wide[:, 300:300 + n] = x
    wide[:, :300] = 7.0
    wide[:, 300 + n:] = -7.0
    rc, s, per, corr = la.cell_search_ant(x, K.NOF_PRB, with_corr=True)
    view = wide[:, 300:300 + n]
    assert view.strides[0] == 8 * (n + 1000)
    rc2, s2, per2, corr2 = la.cell_search_ant(view, K.NOF_PRB, with_corr=True)
    assert rc == rc2 == 1 and bytes(s) == bytes(s2) and [bytes(p) for p in per] == [bytes(p) for p in per2] and np.array_equal(bits(corr), bits(corr2))
    d = torch.from_numpy(wide.view(np.float32)).to("cuda:0").view(torch.complex64)[:, 300:300 + n]
    rc3, s3, per3, corr3 = la.cell_search_ant(d, K.NOF_PRB, with_corr=True)
    assert rc3 == 1 and bytes(s) == bytes(s3) and [bytes(p) for p in per] == [bytes(p) for p in per3] and np.array_equal(bits(corr), bits(corr3))


def test_scan_finds_the_carriers_that_each_antenna_holds_alone(tmp_path):
    """carrier A only on antenna 0, carrier B only on antenna 1: a scan of one antenna reports one carrier (the limit this feature lifts), the scan of all antennas
    both, with the offsets and cells of the one-antenna answers; lsn_file_carrier_scan gives the same on the same bytes"""
    x, truth = K.scan_recording()
    one = [la.carrier_scan(x, K.RATE_SCAN, antenna=a) for a in range(2)]
    for a in range(2):
        assert [(c.center_offset_hz, c.search.cell_id, c.search.cp, c.search.found) for c in one[a]] == [(truth[a]["f_hz"], truth[a]["cell_id"], truth[a]["cp"], 1)], a
    both, metric = la.carrier_scan(x, K.RATE_SCAN, antenna="all", with_metric=True)
    assert sorted(c.center_offset_hz for c in both) == sorted(t["f_hz"] for t in truth)
    for c in both:
        ref = one[0][0] if c.center_offset_hz == truth[0]["f_hz"] else one[1][0]
        assert (c.center_offset_hz, c.k) == (ref.center_offset_hz, ref.k)
        assert [getattr(c.search, f) for f in FIELDS] == [getattr(ref.search, f) for f in FIELDS]
        assert (c.scan_root, c.scan_lag) == (c.search.n_id_2, c.search.pss_pos) and abs(c.scan_p2avg - c.search.pss_p2avg) <= 1e-6 * c.search.pss_p2avg
        # the verification is the search over all antennas on lsn_carrier_channel's samples
        ch = la.carrier_channel(x, K.RATE_SCAN, c.center_offset_hz, n_out=la.carrier_scan_plan(K.RATE_SCAN)["nof_channel_samples"])
        rc, direct, _ = la.cell_search_ant(ch, 6, nof_periods=2)
        assert rc == 1 and bytes(direct) == bytes(c.search)
    path = os.path.join(str(tmp_path), "two.cf32")
    x.tofile(path)
    ffound, fmetric = la.file_carrier_scan(path, K.RATE_SCAN, nof_antennas=2, antenna="all", with_metric=True)
    assert [bytes(c) for c in ffound] == [bytes(c) for c in both] and [bytes(m) for m in fmetric] == [bytes(m) for m in metric]


def test_scan_of_all_antennas_of_a_one_antenna_recording_is_the_scan_of_antenna_0():
    x, _ = K.scan_recording()
    x0 = np.ascontiguousarray(x[:, :1])
    a, am = la.carrier_scan(x0, K.RATE_SCAN, antenna=0, with_metric=True)
    b, bm = la.carrier_scan(x0, K.RATE_SCAN, antenna="all", with_metric=True)
    assert len(a) == 1 and [bytes(c) for c in a] == [bytes(c) for c in b] and [bytes(m) for m in am] == [bytes(m) for m in bm]
    for bad in (2, 0xFFFFFFFE):
        with pytest.raises(RuntimeError):
            la.carrier_scan(x, K.RATE_SCAN, antenna=bad)

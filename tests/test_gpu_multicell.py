"""The successive cell search on the GPU (lsn_cell_search_all; kernels/cells_sync.hip): k_pss_cancel and k_sync_fin_acc against the float64 model of
tests/multicell_model.py within the float32 bounds the model derives, the patched correlation of k_pss_corr_win against a full k_pss_corr of the residual bit for
bit, and the search itself: cell 0 is lsn_cell_search's answer, two co-channel cells are found down to -6 dB in four geometries, nothing but transmitted cells is
reported below that, and each found cell's MIB decodes."""
import ctypes as C
import functools

import numpy as np
import pytest

import ltesniffer_amd as la
import multicell_cases as K
import multicell_model as M
from lsn_testlib import scenario, sync_capture
from parity import gen_subframes

pytestmark = pytest.mark.gpu
INVALID = -2   # LSN_ERROR_INVALID_INPUTS
PRB_OF = {128: 6, 512: 25, 2048: 100}
FIELDS = ("found", "cell_id", "n_id_2", "n_id_1", "sf_idx", "pss_pos", "sf_start", "cp")
FLOATS = ("pss_peak", "pss_p2avg", "sss_metric", "sss_second", "cfo_hz", "cfo_coarse_hz")


def lib_replica(nof_prb, n_id_2, cfo_hz):
    """the replica the library cancels with (lsn_clock_replica; the CPU suite holds it to the model's own)"""
    N = M.SYMBOL[nof_prb]
    cfg = la.ClockCfg(C.sizeof(la.ClockCfg), nof_prb, la.RATES_3GPP, n_id_2, 100, float(cfo_hz), 200.0, 0, 0)
    r = np.zeros(N, dtype=np.complex64)
    assert la.lib().lsn_clock_replica(C.byref(cfg), r.ctypes.data) == 0
    return r


def same_cell(g, o):
    assert [getattr(g, f) for f in FIELDS] == [getattr(o, f) for f in FIELDS], ([getattr(g, f) for f in FIELDS], [getattr(o, f) for f in FIELDS])
    a = np.array([getattr(g, f) for f in FLOATS], dtype=np.float32)
    b = np.array([getattr(o, f) for f in FLOATS], dtype=np.float32)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a, b)


# ---------------- kernels ----------------
@pytest.mark.parametrize("cfo", [0.0, 900.0])
@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("N", [128, 512])
def test_pss_cancel_against_the_model(N, P, cfo):
    """a PSS of root 2 with a gain of its own per occurrence in noise, at a lag 3 samples in front of the end of the 5 ms window: a_j and the residual inside the
    bound multicell_model.cancel derives ((N + 3) 2^-24 times the dot product's sum of magnitudes, through a_j p and the subtraction); two runs give the same
    bits; the input is not written.  Largest error / bound seen on an MI355X: DESIGN 3.1n"""
    W5, prb = 75 * N, PRB_OF[N]
    bn = W5 - 3
    rng = np.random.default_rng(N + P)
    n = (P + 1) * W5 + N + 17
    x = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))    # the projection of this noise on the replica: 0.014 rms
    p = lib_replica(prb, 2, cfo)
    gains = rng.standard_normal(P + 1) + 1j * rng.standard_normal(P + 1)
    for j in range(P + 1):
        x[bn + j * W5:bn + j * W5 + N] += gains[j] * p
    x = x.astype(np.complex64)
    keep = x.copy()
    res, a = la.pss_cancel(x, prb, 2, bn, cfo_hz=cfo, nof_periods=P)
    assert np.array_equal(x.view(np.uint32), keep.view(np.uint32))
    want, wa, br, ba = M.cancel(x, p, N, P, bn, with_bound=True)
    ea = np.stack([np.abs(a.real - wa.real), np.abs(a.imag - wa.imag)], axis=1)
    assert np.all(ea <= ba), (ea / ba).max()
    touched = br[:, 0] > 0
    assert touched.sum() == (P + 1) * N and np.array_equal(res[~touched].view(np.uint32), x[~touched].view(np.uint32))
    er = np.stack([np.abs(res.real - want.real), np.abs(res.imag - want.imag)], axis=1)
    assert np.all(er[touched] <= br[touched]), (er[touched] / br[touched]).max()
    print("k_pss_cancel N %d P %d cfo %g: largest error / bound  a_j %.4f  residual %.4f" % (N, P, cfo, (ea / ba).max(), (er[touched] / br[touched]).max()))
    assert np.all(np.abs(wa - gains) < 0.1)
    res2, a2 = la.pss_cancel(x, prb, 2, bn, cfo_hz=cfo, nof_periods=P)
    assert np.array_equal(res.view(np.uint32), res2.view(np.uint32)) and np.array_equal(a.view(np.uint32), a2.view(np.uint32))


def _capture_with_pss_at(nof_prb, target, periods, cell_id=301, cfo_hz=900.0):
    """one cell whose first PSS sits at lag `target` of the 5 ms window"""
    N = M.SYMBOL[nof_prb]
    W5 = 75 * N
    lead = (target - 2 * 15 * N - M.pss_offset(N, 0)) % W5   # the capture starts with subframe 3: the first PSS is in subframe 5
    sc = scenario("small", seed=5, start_tti=773, nof_prb=nof_prb, cell_id=cell_id, cfo_hz=cfo_hz)
    x, _ = sync_capture(sc, lead, periods)
    return x


@pytest.mark.parametrize("N,P,where", [(128, 8, "front"), (128, 8, "end"), (512, 8, "front"), (512, 8, "end"), (512, 8, "two"), (2048, 1, "end")])
def test_patched_correlation_equals_a_full_one_of_the_residual(N, P, where):
    """round 1's correlation of cell_search_all - round 0's with 2 N - 1 lags recomputed by k_pss_corr_win - against k_pss_corr over all 75 N lags of the residual
    that lsn_pss_cancel leaves: every bit.  front / end: the window wraps at lag 0 / at 75 N; two: the two-cell capture, window in mid-range"""
    prb, W5 = PRB_OF[N], 75 * N
    x = K.two_cells(304, 9000, -3.0) if where == "two" else _capture_with_pss_at(prb, 5 if where == "front" else W5 - 3, P)
    rc, s0 = la.cell_search(x, prb, nof_periods=P)
    assert rc == 1
    plan = la.cell_search_all_plan(s0.pss_pos, N)
    assert len(plan["runs"]) == (1 if where == "two" else 2)
    res, _ = la.pss_cancel(x, prb, s0.n_id_2, s0.pss_pos, cfo_hz=s0.cfo_hz, nof_periods=P)
    _, _, full = la.cell_search(res, prb, nof_periods=P, with_corr=True)
    cells, corr = la.cell_search_all(x, prb, nof_periods=P, threshold_next=8.0 if P == 8 else 25.0, with_corr=True)
    assert len(corr) >= 2 and len(cells) >= 1
    assert np.array_equal(corr[1].view(np.uint32), full.view(np.uint32)), int((corr[1] != full).sum())
    _, _, first = la.cell_search(x, prb, nof_periods=P, with_corr=True)
    assert np.array_equal(corr[0].view(np.uint32), first.view(np.uint32))
    lags = M.window_lags(s0.pss_pos, N)
    outside = np.ones(W5, dtype=bool)
    outside[lags] = False
    assert np.array_equal(corr[1][:, outside].view(np.uint32), corr[0][:, outside].view(np.uint32)) and corr[1][s0.n_id_2, s0.pss_pos] < 0.05 * s0.pss_peak


def test_accumulated_sss_against_the_model():
    """the lone cell A: the 336 coherent sums of every occurrence under both CP hypotheses - the occurrence k_sync_fin takes among them - and the accumulated
    powers, inside the bounds multicell_model.sss_occurrence / sss_accumulate carry through the DFTs, the channel, its average and the sums"""
    x = K.cell_a()
    rc, s = la.cell_search(x, K.NOF_PRB, nof_periods=K.PERIODS)
    assert rc == 1 and s.cell_id == 301
    got = la.sss_accumulate(x, K.NOF_PRB, s.n_id_2, s.pss_pos, nof_periods=K.PERIODS)
    A = M.sss_accumulate(x, M.replica(s.n_id_2, K.N), K.N, K.PERIODS, s.n_id_2, s.pss_pos)
    worst = 0.0
    for cp in range(2):
        for j, o in enumerate(A["occ"][cp]):
            assert bool(got["valid"][cp, j]) == o["valid"]
            if not o["valid"]:
                continue
            g = got["sums"][cp, j]
            e = np.maximum(np.abs(g.real - o["sums"].real), np.abs(g.imag - o["sums"].imag))
            assert np.all(e <= o["bound"]), (cp, j, (e / o["bound"]).max())
            worst = max(worst, float((e / o["bound"]).max()))
    jb = M.strongest(A["occ"][0])
    h = 2 * s.n_id_1 + (1 if (s.sf_idx == 5) != (s.pss_pos < M.pss_offset(K.N, 0)) else 0)
    assert int(np.argmax(np.abs(got["sums"][0, jb]) ** 2)) == h ^ (jb & 1) and int(np.argmax(got["acc"][0])) == h
    ea = np.abs(got["acc"].astype(np.float64) - A["acc"])
    assert np.all(ea <= A["acc_bound"]), (ea / A["acc_bound"]).max()
    print("k_sync_fin_acc: largest error / bound  sums %.4f  accumulated powers %.4f" % (worst, (ea / A["acc_bound"]).max()))
    hv = got["halves"]
    for j, o in enumerate(A["occ"][0]):
        if o["valid"]:
            assert np.allclose(hv[j, :, 0] + 1j * hv[j, :, 1], o["y"], rtol=0, atol=1e-4 * np.abs(o["y"]).max() + 1e-6) and np.allclose(hv[j, :, 2], o["e"], rtol=1e-4)


# ---------------- the search ----------------
@functools.lru_cache(maxsize=None)
def _search(cell_b, lead_b, amp_db):
    x = K.cell_a() if cell_b is None else K.two_cells(cell_b, lead_b, amp_db)
    return x, la.cell_search_all(x, K.NOF_PRB, nof_periods=K.PERIODS)


def _cell0_is_the_one_cell_search(x, cells):
    import torch
    rc, s = la.cell_search(x, K.NOF_PRB, nof_periods=K.PERIODS)
    assert bool(rc) == bool(cells)
    if cells:
        same_cell(cells[0].cell, s)
        assert cells[0].round == 0 and cells[0].shared_pss == 0 and cells[0].rel_power_db == 0.0
    xd = torch.from_numpy(np.array(x, dtype=np.complex64).view(np.float32)).to("cuda:0")   # (a copy: the shared captures are read-only)
    again = la.cell_search_all(xd.view(torch.complex64), K.NOF_PRB, nof_periods=K.PERIODS)
    assert [bytes(c) for c in again] == [bytes(c) for c in cells]            # samples already in device memory: the same list
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), np.ascontiguousarray(x).view(np.uint32).reshape(-1))   # and never written


def _check_transmitted(cells, want):
    ids = [c.cell.cell_id for c in cells]
    assert len(set(ids)) == len(ids)
    for c in cells:
        assert c.cell.cell_id in want, (ids, want)
        start, sf = want[c.cell.cell_id]
        assert c.cell.cp == 0 and c.cell.sf_idx == sf and abs(int(c.cell.sf_start) - start) <= (0 if c.round == 0 else 1), (c.cell.cell_id, c.cell.sf_start, start)


@pytest.mark.parametrize("amp_db", K.AMPLITUDES_DB)
@pytest.mark.parametrize("cell_b,lead_b", K.GEOMETRIES)
def test_two_cells_are_found(cell_b, lead_b, amp_db):
    x, cells = _search(cell_b, lead_b, amp_db)
    print([(c.cell.cell_id, c.cell.sf_start, c.round, round(c.sss_ratio, 2), round(c.cell.pss_p2avg, 1), round(c.rel_power_db, 2), round(c.cell.cfo_hz, 1)) for c in cells])
    _cell0_is_the_one_cell_search(x, cells)
    _check_transmitted(cells, K.transmitted(cell_b, lead_b))
    assert len(cells) == 2 and [c.shared_pss for c in cells] == [0, 0] and [c.round for c in cells] == [0, 1]
    weak = cells[1]
    assert weak.rel_power_db <= 0.5 and abs(abs(weak.rel_power_db) - abs(amp_db)) <= 1.5, weak.rel_power_db
    assert weak.sss_ratio >= 1.5 and weak.cell.pss_p2avg >= 8.0
    # the weaker cell's carrier offset against the model's, evaluated on the residual the library's cancellation of cell 0 leaves
    c0 = cells[0].cell
    res, _ = la.pss_cancel(x, K.NOF_PRB, c0.n_id_2, c0.pss_pos, cfo_hz=c0.cfo_hz, nof_periods=K.PERIODS)
    A = M.sss_accumulate(res, M.replica(weak.cell.n_id_2, K.N), K.N, K.PERIODS, weak.cell.n_id_2, weak.cell.pss_pos)
    d = M.decide(1, 1.0, 1.0, 1, A["acc"])
    m = M.cell_from(K.N, weak.cell.n_id_2, weak.cell.pss_pos, d["cp"], d["best"], A, with_bound=True)
    assert (m["cell_id"], m["cp"], m["sf_start"], m["sf_idx"]) == (weak.cell.cell_id, weak.cell.cp, weak.cell.sf_start, weak.cell.sf_idx)
    assert abs(weak.cell.cfo_hz - m["cfo_hz"]) <= m["cfo_bound"], (weak.cell.cfo_hz, m["cfo_hz"], m["cfo_bound"])
    assert abs(weak.sss_ratio - d["sss_ratio"]) <= 1e-3 * d["sss_ratio"]
    sent = {K.CELL_A["cell_id"]: K.CELL_A["cfo_hz"], cell_b: -400.0}
    print("cfo_hz - transmitted:", [(c.cell.cell_id, round(c.cell.cfo_hz - sent[c.cell.cell_id], 1)) for c in cells], " model bound %.3g Hz" % m["cfo_bound"])


@pytest.mark.parametrize("amp_db", K.WEAK_DB)
@pytest.mark.parametrize("cell_b,lead_b", K.GEOMETRIES)
def test_a_weak_second_cell_adds_nothing_that_was_not_transmitted(cell_b, lead_b, amp_db):
    x, cells = _search(cell_b, lead_b, amp_db)
    _cell0_is_the_one_cell_search(x, cells)
    _check_transmitted(cells, K.transmitted(cell_b, lead_b))
    assert cells and cells[0].cell.cell_id == K.CELL_A["cell_id"]


def test_one_cell_noise_and_two_cells_on_one_pss():
    x, cells = _search(None, None, None)
    _cell0_is_the_one_cell_search(x, cells)
    _check_transmitted(cells, K.transmitted())
    assert len(cells) == 1 and cells[0].sss_ratio >= 2.0
    assert la.cell_search_all(K.noise(), K.NOF_PRB, nof_periods=K.PERIODS) == []
    _cell0_is_the_one_cell_search(K.noise(), [])
    x = K.two_cells(*K.SHARED, 0.0)
    cells = la.cell_search_all(x, K.NOF_PRB, nof_periods=K.PERIODS)
    _cell0_is_the_one_cell_search(x, cells)
    _check_transmitted(cells, K.transmitted(*K.SHARED))
    assert len(cells) == 2 and [c.shared_pss for c in cells] == [0, 1] and [c.round for c in cells] == [0, 0]
    assert cells[1].cell.pss_pos == cells[0].cell.pss_pos and cells[0].sss_ratio < 1.5
    off = la.cell_search_all(x, K.NOF_PRB, nof_periods=K.PERIODS, shared_pss_ratio=-1.0)
    assert len(off) == 1 and bytes(off[0].cell) == bytes(cells[0].cell)
    one = la.cell_search_all(K.two_cells(304, 9000, -3.0), K.NOF_PRB, nof_periods=K.PERIODS, max_cells=1)
    assert len(one) == 1 and one[0].cell.cell_id == 301


@pytest.mark.parametrize("amp_db", [0.0, -6.0])
def test_each_found_cells_mib_decodes(amp_db):
    """two-antenna streams of 50 subframes, A (301, from TTI 7733) plus B (304, from TTI 5011) 7767 samples later: the search on antenna 0, then one 25-block Phy
    per found cell decodes the MIB of that cell's first transmitted subframe 0 at the timing the search gave, with the SFN that subframe carries"""
    sflen, nsf, delay = K.SFLEN, 50, 7767
    streams = []
    for cid, seed, tti, cfo in ((301, 5, 7733, 900.0), (304, 6, 5011, -400.0)):
        sc = scenario("small", seed=seed, start_tti=tti, nof_prb=K.NOF_PRB, cell_id=cid, cfo_hz=cfo)
        tti0, iq, _ = gen_subframes(sc, nsf)
        assert tti0 == tti
        streams.append(np.concatenate(list(iq), axis=1))
    x = streams[0].copy()
    x[:, delay:] += np.float32(10.0 ** (amp_db / 20.0)) * streams[1][:, :nsf * sflen - delay]
    cells = la.cell_search_all(x[0], K.NOF_PRB, nof_periods=K.PERIODS)
    assert sorted(c.cell.cell_id for c in cells) == [301, 304], [(c.cell.cell_id, c.round, c.sss_ratio) for c in cells]
    first = {301: (0, 7733), 304: (delay, 5011)}
    for c in cells:
        t0, tti = first[c.cell.cell_id]
        start = int(c.cell.sf_start) + (0 if c.cell.sf_idx == 0 else 5 * sflen)
        while start < t0:                                   # in front of the cell's first sample nothing of it is on the air
            start += 10 * sflen
        assert (start - t0) % sflen in (0, 1, sflen - 1)
        sf_tti = tti + int(round((start - t0) / sflen))
        assert sf_tti % 10 == 0
        phy = la.Phy(nof_rx_antennas=2, max_batch=1, pcapwriter=la.PcapWriter(None))
        try:
            assert phy.setCell(K.NOF_PRB, 2, int(c.cell.cell_id), cp=int(c.cell.cp))
            m = phy.mib_decode(x[:, start:start + sflen])
            assert m["found"] and m["nof_prb"] == K.NOF_PRB and m["nof_ports"] == 2, (c.cell.cell_id, m)
            assert m["sfn"] == (sf_tti // 10) % 1024, (c.cell.cell_id, m, sf_tti)
        finally:
            phy.close()


def test_carrier_cells_is_the_channel_then_the_search():
    import scan_model as SM
    x, truth = SM.two_cell_recording()
    found = la.carrier_scan(x, SM.RATE_TWO)
    assert len(found) == 2
    kw = dict(nof_periods=2, threshold_next=25.0)          # the scan's two periods: threshold_next is measured for 8 and must be raised
    for c in found:
        cells = la.carrier_cells(x, SM.RATE_TWO, c.center_offset_hz, **kw)
        ch = la.carrier_channel(x, SM.RATE_TWO, c.center_offset_hz)
        assert [bytes(k) for k in cells] == [bytes(k) for k in la.cell_search_all(ch[0], 6, **kw)]
        assert len(cells) == 1 and bytes(cells[0].cell) == bytes(c.search)       # one cell per carrier in this recording: the scan's


def test_refusals():
    L = la.lib()
    x = K.noise()
    out = (la.CellFound * 8)()
    nf = C.c_uint32(7)

    def rc(nof_prb=K.NOF_PRB, n=x.size, ptr=x.ctypes.data, device=0, found=C.byref(nf), cells=out, **kw):
        f = dict(nof_periods=8, force_n_id_2=-1, threshold=20.0, threshold_next=0.0, sss_ratio_min=0.0, shared_pss_ratio=0.0, max_cells=0)
        f.update(kw)
        cfg = la.CellSearchAllCfg(f["nof_periods"], f["force_n_id_2"], f["threshold"], f["threshold_next"], f["sss_ratio_min"], f["shared_pss_ratio"], f["max_cells"])
        return L.lsn_cell_search_all(device, ptr, 0, n, nof_prb, la.RATES_3GPP, C.byref(cfg), cells, found, None)

    assert rc() == 0 and nf.value == 0
    assert rc(nof_periods=0) == 0                           # 0 = 8 periods
    for bad in (dict(nof_prb=70), dict(n=x.size - 1), dict(nof_periods=9), dict(max_cells=9), dict(nof_periods=17), dict(threshold=float("nan")),
                dict(threshold_next=float("inf")), dict(sss_ratio_min=float("nan")), dict(shared_pss_ratio=float("inf")), dict(force_n_id_2=3), dict(ptr=None),
                dict(found=None), dict(cells=None)):
        assert rc(**bad) == INVALID, bad
    assert rc(device=99) == la.LSN_ERROR_NO_DEVICE
    with pytest.raises(RuntimeError):
        la.cell_search_all(x, K.NOF_PRB, nof_periods=8, max_cells=9)
    res = np.zeros_like(x)
    a = np.zeros(9, dtype=np.complex64)

    def rcc(n_id_2=0, pos=0, cfo=0.0, P=8, n=x.size, r=res.ctypes.data):
        return L.lsn_pss_cancel(0, x.ctypes.data, n, K.NOF_PRB, la.RATES_3GPP, P, n_id_2, pos, cfo, r, a.ctypes.data)

    assert rcc() == 0
    assert rcc(n_id_2=3) == INVALID and rcc(pos=K.W5) == INVALID and rcc(cfo=float("nan")) == INVALID and rcc(P=0) == INVALID and rcc(P=17) == INVALID
    assert rcc(n=x.size - 1) == INVALID and rcc(r=None) == INVALID
    forced = la.cell_search_all(K.cell_a(), K.NOF_PRB, force_n_id_2=1)
    assert len(forced) == 1 and forced[0].cell.cell_id == 301
    rc1, s1 = la.cell_search(K.cell_a(), K.NOF_PRB, nof_periods=8, force_n_id_2=1)
    same_cell(forced[0].cell, s1)

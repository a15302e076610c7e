"""The successive cell search without a GPU: the float64 model of tests/multicell_model.py finds the transmitted cells on every capture
the GPU tests use, lsn_cell_search_all_plan and lsn_cell_search_all_decide equal the model's window and rule, a cancellation changes the correlation only inside
the window, and the new symbols exist in the library and its C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ltesniffer_amd as la
import multicell_cases as K
import multicell_model as M

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
NEW = ["lsn_cell_search_all", "lsn_pss_cancel", "lsn_sss_accumulate", "lsn_cell_search_all_plan", "lsn_cell_search_all_decide"]


def test_new_symbols_exist_and_the_cpp_mirror_compiles():
    for s in NEW:
        assert s in la.EXPORTS
        getattr(la.lib(), s)
    for f in ("cell_search_all", "pss_cancel", "cell_search_all_plan", "cell_search_all_decide", "carrier_cells"):
        assert callable(getattr(la, f))
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
    hpp = open(os.path.join(d, "..", "..", "include", "ltesniffer_amd.hpp")).read()
    assert "cellSearchAll" in hpp and "lsn_cell_search_all" in hpp
    subprocess.check_call(["make", "-C", d, "_build/test_hpp"], stdout=subprocess.DEVNULL)   # includes the mirror, links the library: as tests/test_cabi_and_oracle.py
    assert C.sizeof(la.CellFound) == C.sizeof(la.CellSearch) + 16 and C.sizeof(la.CellSearchAllCfg) == 28


def _check_cells(cells, want, n_expected=None):
    ids = [c["cell_id"] for c in cells]
    assert len(set(ids)) == len(ids)
    for c in cells:
        assert c["cell_id"] in want, (ids, want)
        start, sf = want[c["cell_id"]]
        assert c["cp"] == 0 and abs(c["sf_start"] - start) <= (0 if c["round"] == 0 else 1) and c["sf_idx"] == sf, (c, want)
    if n_expected is not None:
        assert len(cells) == n_expected, (ids, want)


@pytest.mark.parametrize("amp_db", K.AMPLITUDES_DB)
@pytest.mark.parametrize("cell_b,lead_b", K.GEOMETRIES)
def test_model_finds_both_cells(cell_b, lead_b, amp_db):
    cells = M.search_all(K.two_cells(cell_b, lead_b, amp_db), K.NOF_PRB)
    print([(c["cell_id"], c["sf_start"], round(c["sss_ratio"], 2), round(c["p2avg"], 1), round(c["rel_power_db"], 2), round(c["cfo_hz"])) for c in cells])
    _check_cells(cells, K.transmitted(cell_b, lead_b), 2)
    assert abs(abs(cells[1]["rel_power_db"]) - abs(amp_db)) <= 1.5 and cells[1]["rel_power_db"] <= 0.5
    assert all(c["shared_pss"] == 0 for c in cells)


@pytest.mark.parametrize("amp_db", K.WEAK_DB)
@pytest.mark.parametrize("cell_b,lead_b", K.GEOMETRIES)
def test_model_reports_only_transmitted_cells_when_the_second_is_weak(cell_b, lead_b, amp_db):
    cells = M.search_all(K.two_cells(cell_b, lead_b, amp_db), K.NOF_PRB)
    _check_cells(cells, K.transmitted(cell_b, lead_b))
    assert cells and cells[0]["cell_id"] == K.CELL_A["cell_id"]


def test_model_one_cell_noise_and_a_shared_pss():
    _check_cells(M.search_all(K.cell_a(), K.NOF_PRB), K.transmitted(), 1)
    assert M.search_all(K.noise(), K.NOF_PRB) == []
    cells = M.search_all(K.two_cells(*K.SHARED, 0.0), K.NOF_PRB)
    _check_cells(cells, K.transmitted(*K.SHARED), 2)
    assert [c["shared_pss"] for c in cells] == [0, 1] and cells[0]["round"] == cells[1]["round"] == 0
    assert cells[0]["sss_ratio"] < 1.5                         # two equal cells on one PSS: best / second near 1
    assert len(M.search_all(K.two_cells(*K.SHARED, 0.0), K.NOF_PRB, shared_pss_ratio=-1.0)) == 1


@pytest.mark.parametrize("N", [128, 512, 2048])
def test_plan_equals_the_models_window(N):
    W5 = 75 * N
    for bn in (0, N - 1, W5 - N, W5 - 1, W5 // 2 + 7, N, N - 2, W5 - N + 1):
        got, want = la.cell_search_all_plan(bn, N), M.window(bn, N)
        assert got == want, (bn, got, want)
        lags = np.concatenate([lo + np.arange(n) for lo, n in got["runs"]])
        assert np.array_equal(lags, M.window_lags(bn, N)) and len(set(lags.tolist())) == 2 * N - 1
        assert all(lo + n <= W5 for lo, n in got["runs"])
        d = (lags - bn + W5 // 2) % W5 - W5 // 2
        assert np.abs(d).max() == N - 1                        # exactly the lags with |n - bn| < N modulo W5
    pl = la.CellSearchAllPlan()
    L = la.lib()
    assert L.lsn_cell_search_all_plan(W5, N, W5, C.byref(pl)) == INVALID
    assert L.lsn_cell_search_all_plan(0, 0, W5, C.byref(pl)) == INVALID
    assert L.lsn_cell_search_all_plan(0, N, W5, None) == INVALID


@pytest.mark.parametrize("bn", [0, 127, 9600 - 128, 9599, 4801])
def test_a_cancellation_changes_the_correlation_only_inside_the_window(bn):
    """6 resource blocks, 2 periods, a PSS of root 1 planted at bn in noise: the full float64 correlation after the cancellation differs from the one before
    at no lag outside the model's window, and does differ inside it"""
    N, P = 128, 2
    W5 = 75 * N
    rng = np.random.default_rng(bn)
    n = (P + 1) * W5 + N
    x = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    p = M.replica(1, N, 300.0).astype(np.complex128)
    for j in range(P + 1):
        x[bn + j * W5:bn + j * W5 + N] += (1.0 + 0.2j) * p
    x = x.astype(np.complex64)
    reps = [M.replica(r, N) for r in range(3)]
    res, a = M.cancel(x, p, N, P, bn)
    assert np.all(np.abs(a - (1.0 + 0.2j)) < 0.02)
    changed = np.flatnonzero(res != x.astype(np.complex128))
    assert changed.min() >= bn and changed.max() < bn + P * W5 + N
    lags = np.arange(W5)
    before, after = M.corr_direct(x, reps, N, P, lags), M.corr_direct(res, reps, N, P, lags)
    inside = np.zeros(W5, dtype=bool)
    inside[M.window_lags(bn, N)] = True
    assert np.array_equal(before[:, ~inside], after[:, ~inside])
    assert np.all(np.any(before[:, inside] != after[:, inside], axis=1))
    assert before[1, bn] > 0.9 * P and after[1, bn] < 0.05 * before[1, bn]
    assert np.allclose(M.corr_full(x, reps, N, P), before, rtol=1e-9, atol=1e-12)


def _acc(best=None, powers=(), cp=0, floor=1.0):
    a = np.full((2, 336), floor * 0.1, dtype=np.float32)
    a[cp] = floor
    for h, v in powers:
        a[cp, h] = v
    return a


def _same(got, want):
    for f in ("accept", "cp", "best", "second", "runner_up", "shared"):
        assert int(getattr(got, f)) == int(want[f]), (f, getattr(got, f), want)
    assert abs(got.p2avg - want["p2avg"]) <= 1e-6 * want["p2avg"] and abs(got.sss_ratio - want["sss_ratio"]) <= 1e-6 * max(want["sss_ratio"], 1.0)


def test_decide_equals_the_model_on_recorded_statistics():
    W5 = 38400
    rows = [
        # round, peak, sum, accumulated powers                                               what it shows
        (1, 1.2, 0.1 * W5, _acc(powers=[(202, 9.0), (77, 3.0)])),                            # accepted: p2avg 12, ratio 3
        (1, 0.79, 0.1 * W5, _acc(powers=[(202, 9.0), (77, 3.0)])),                           # the stop: p2avg 7.9 under threshold_next
        (1, 1.2, 0.1 * W5, _acc(powers=[(202, 9.0), (77, 6.1)])),                            # the stop: ratio 1.475 under sss_ratio_min
        (2, 1.2, 0.1 * W5, _acc(powers=[(202, 9.0), (77, 5.9)])),                            # accepted, and 77 is a cell of its own (0.655 of the best)
        (1, 1.2, 0.1 * W5, _acc(powers=[(202, 9.0), (203, 5.9), (77, 5.0)])),                # the other-half-frame twin 203 is second, never the runner-up
        (1, 1.2, 0.1 * W5, _acc(powers=[(202, 9.0), (203, 5.9), (77, 5.5)])),                # ... and 77 behind it still qualifies as shared
        (0, 1.9, 0.1 * W5, _acc(powers=[(10, 9.0), (300, 8.7)])),                            # round 0: under the threshold of 20
        (0, 2.1, 0.1 * W5, _acc(powers=[(10, 9.0), (300, 8.7)])),                            # round 0: accepted whatever the ratio, shared PSS
        (1, 1.2, 0.1 * W5, _acc(powers=[(5, 9.0), (77, 3.0)], cp=1)),                        # extended CP wins
        (1, 1.2, 0.1 * W5, _acc(powers=[(202, 9.0), (20, 9.0), (77, 3.0)])),                 # equal powers: the first maximum is the best
    ]
    for rnd, peak, total, acc in rows:
        _same(la.cell_search_all_decide(rnd, peak, total, W5, acc), M.decide(rnd, peak, total, W5, acc))
    assert [la.cell_search_all_decide(r, p, t, W5, a).accept for r, p, t, a in rows] == [1, 0, 0, 1, 1, 1, 0, 1, 1, 0]
    assert [la.cell_search_all_decide(r, p, t, W5, a).shared for r, p, t, a in rows] == [0, 0, 1, 1, 0, 1, 1, 1, 0, 1]
    d = la.cell_search_all_decide(1, 1.2, 0.1 * W5, W5, rows[4][3])
    assert (d.best, d.second, d.runner_up) == (202, 203, 77)
    # a tie between the CP hypotheses: normal
    tie = _acc(powers=[(202, 9.0)])
    tie[1] = tie[0]
    assert la.cell_search_all_decide(1, 1.2, 0.1 * W5, W5, tie).cp == 0 and M.decide(1, 1.2, 0.1 * W5, W5, tie)["cp"] == 0
    # other settings: thresholds, and the shared-PSS rule switched off
    acc = rows[3][3]
    kw = dict(threshold_next=12.5, sss_ratio_min=1.2, shared_pss_ratio=0.7)
    _same(la.cell_search_all_decide(2, 1.2, 0.1 * W5, W5, acc, **kw), M.decide(2, 1.2, 0.1 * W5, W5, acc, **kw))
    assert la.cell_search_all_decide(2, 1.2, 0.1 * W5, W5, acc, shared_pss_ratio=-1.0).shared == 0
    # the model's own statistics on a capture go through the product's rule unchanged
    x = K.two_cells(304, 9000, -6.0)
    cells, corrs = M.search_all(x, K.NOF_PRB, with_corr=True)
    for rnd, Cm in enumerate(corrs):
        root = int(np.argmax(Cm.max(axis=1)))
        bn = int(np.argmax(Cm[root]))
        r = x.astype(np.complex128)
        for c in cells[:rnd]:
            r, _ = M.cancel(r, M.replica(c["n_id_2"], K.N, c["cfo_hz"]), K.N, K.PERIODS, c["pss_pos"])
        A = M.sss_accumulate(r, M.replica(root, K.N), K.N, K.PERIODS, root, bn)
        _same(la.cell_search_all_decide(rnd, Cm[root, bn], Cm[root].sum(), K.W5, A["acc"]), M.decide(rnd, Cm[root, bn], Cm[root].sum(), K.W5, A["acc"]))
    assert len(corrs) == 3 and len(cells) == 2


def test_decide_refusals():
    L = la.lib()
    out = la.CellSearchAllDecision()
    acc = _acc()

    def rc(**kw):
        f = dict(nof_periods=8, force_n_id_2=-1, threshold=20.0, threshold_next=0.0, sss_ratio_min=0.0, shared_pss_ratio=0.0, max_cells=0)
        f.update(kw)
        cfg = la.CellSearchAllCfg(f["nof_periods"], f["force_n_id_2"], f["threshold"], f["threshold_next"], f["sss_ratio_min"], f["shared_pss_ratio"], f["max_cells"])
        return L.lsn_cell_search_all_decide(C.byref(cfg), 1, 1.0, 100.0, 9600, acc.ctypes.data, C.byref(out))

    assert rc() == 0 and rc(max_cells=8, nof_periods=16) == 0
    for bad in (dict(max_cells=9), dict(nof_periods=17), dict(threshold=float("nan")), dict(threshold_next=float("inf")), dict(sss_ratio_min=float("nan")),
                dict(shared_pss_ratio=float("nan")), dict(force_n_id_2=3), dict(threshold_next=-1.0)):
        assert rc(**bad) == INVALID, bad
    assert L.lsn_cell_search_all_decide(None, 1, 1.0, 100.0, 9600, acc.ctypes.data, C.byref(out)) == INVALID

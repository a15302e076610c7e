"""The cell search over all receive antennas without a GPU: the float64 model of tests/sync_ant_model.py takes the oracle's decisions with
one antenna, finds a cell whose two channels are opposite (where the SUM of the antennas holds nothing), a cell that is absent from antenna 0, and a cell whose SSS
neither antenna decides alone; the noise floor of the combined metric is measured; lsn_cell_search_ant refuses what it must before it looks for a device, and the
scan's plan does not depend on which antennas are scanned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ltesniffer_amd as la
import sync_ant_cases as K
import sync_ant_model as M
from test_sync_oracle import oracle_cell_search

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
SSS_SNRS, SSS_SEEDS = [-6.0 - k for k in range(10)], range(20)   # 200 candidates at falling SNR


def test_new_symbol_exists_and_the_cpp_mirror_compiles():
    assert "lsn_cell_search_ant" in la.EXPORTS
    getattr(la.lib(), "lsn_cell_search_ant")
    assert callable(la.cell_search_ant) and la.SCAN_ALL_ANTENNAS == 0xFFFFFFFF and la.SEARCH_MAX_ANTENNAS == 2
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
    root = os.path.join(d, "..", "..")
    hpp = open(os.path.join(root, "include", "ltesniffer_amd.hpp")).read()
    hdr = open(os.path.join(root, "include", "ltesniffer_amd.h")).read()
    assert "cellSearchAnt" in hpp and "lsn_cell_search_ant" in hpp
    assert "#define LSN_SCAN_ALL_ANTENNAS 0xFFFFFFFFu" in hdr and "#define LSN_SEARCH_MAX_ANTENNAS 2" in hdr
    subprocess.check_call(["make", "-C", d, "_build/test_hpp"], stdout=subprocess.DEVNULL)   # includes the mirror, links the library: as tests/test_cabi_and_oracle.py
    assert C.sizeof(la.CellSearchAnt) == 24 and C.sizeof(la.CarrierScanCfg) == C.sizeof(la.carrier_scan_cfg(7.68e6, antenna="all"))


def _right(m, cell_id=77, cp=0):
    return bool(m["found"]) and m["cell_id"] == cell_id and m["cp"] == cp and (m["sf_start"], m["sf_idx"]) == K.timing()


@pytest.mark.parametrize("cp", [0, 1])
def test_model_with_one_antenna_takes_the_oracles_decisions(cp):
    x = K.clean_cell(cp=cp)
    m = M.search(x, K.NOF_PRB, 2)
    r, s, _ = oracle_cell_search(x, K.NOF_PRB, 2, -1, 20.0)
    assert r == 1 and _right(m, cp=cp)
    for f in ("found", "cell_id", "n_id_2", "n_id_1", "sf_idx", "pss_pos", "sf_start", "cp"):
        assert int(m[f]) == getattr(s, f), f
    for f in ("pss_peak", "pss_p2avg", "sss_metric", "sss_second"):
        assert abs(m[f] - getattr(s, f)) <= 1e-4 * abs(m[f]), (f, m[f], getattr(s, f))
    assert abs(m["cfo_hz"] - s.cfo_hz) <= m["cfo_bound"] and abs(m["cfo_coarse_hz"] - s.cfo_coarse_hz) < 0.5
    p = m["per_ant"][0]
    assert p["pss_peak"] == m["pss_peak"] and p["sss_metric"] == m["sss_metric"] and p["n_id_1"] == m["n_id_1"]


def test_opposite_channels_defeat_the_sum_of_the_antennas_and_not_the_combination():
    x = K.opposite()
    m = M.search(x, K.NOF_PRB, 2)
    print("opposite channels: combined p2avg %.2f, antennas' own peaks %s" % (m["pss_p2avg"], [round(p["pss_peak"], 3) for p in m["per_ant"]]))
    assert _right(m) and abs(m["cfo_hz"] - 700.0) < 150.0
    summed = M.search(x[0].astype(np.complex128) + x[1].astype(np.complex128), K.NOF_PRB, 2)
    print("the same model on antenna 0 + antenna 1: p2avg %.2f" % summed["pss_p2avg"])
    assert not summed["found"] and summed["pss_p2avg"] < 20.0


def test_cell_absent_from_antenna_0_is_found_by_the_combination_only():
    x = K.faded()
    alone = M.search(x[0], K.NOF_PRB, 2)
    m = M.search(x, K.NOF_PRB, 2)
    print("faded: antenna 0 alone p2avg %.2f, combined %.2f, own peaks %s" % (alone["pss_p2avg"], m["pss_p2avg"], [round(p["pss_peak"], 3) for p in m["per_ant"]]))
    assert not alone["found"]
    assert _right(m)
    assert m["per_ant"][1]["pss_peak"] > 10.0 * m["per_ant"][0]["pss_peak"]


def sss_qualifies(snr_db, seed):
    """each antenna's own SSS decision is wrong or ambiguous (best / second < 1.2), the combined one is right and not ambiguous"""
    m = M.search(K.sss_case(snr_db, seed), K.NOF_PRB, 2)
    alone = [p["n_id_1"] != 77 // 3 or p["sss_metric"] < 1.2 * p["sss_second"] for p in m["per_ant"]]
    return all(alone) and _right(m) and m["sss_metric"] >= 1.2 * m["sss_second"], m


def sss_candidates():
    """the search that chose sync_ant_cases.SSS_CASE: the first candidate that qualifies (run by hand: python tests/test_sync_ant_model.py)"""
    for snr in SSS_SNRS:
        for seed in SSS_SEEDS:
            ok, m = sss_qualifies(snr, seed)
            if ok:
                return snr, seed
    return None


def test_sss_decision_that_neither_antenna_takes_alone():
    assert K.SSS_CASE is not None and K.SSS_CASE[0] in SSS_SNRS and K.SSS_CASE[1] in SSS_SEEDS
    ok, m = sss_qualifies(*K.SSS_CASE)
    print("SSS case %s: combined best / second %.2f; per antenna (N_id_1, best / second) %s" %
          (K.SSS_CASE, m["sss_metric"] / m["sss_second"], [(p["n_id_1"], round(p["sss_metric"] / p["sss_second"], 2)) for p in m["per_ant"]]))
    assert ok


def test_noise_floor_of_the_combined_metric_is_measured():
    """a measurement for choosing thresholds, not a pass mark (DESIGN 3.1r records it next to "noise alone stays below 15"); the only assertion is that two
    antennas' noise stays under the documented threshold of 20"""
    reps = [M.MM.replica(r, K.N) for r in range(3)]
    for P in (1, 2, 8):
        worst = 0.0
        for seed in range(50):
            Cn, _ = M.correlation(K.noise(2, P, 100 + seed), reps, K.N, P)
            r, n = divmod(int(np.argmax(Cn.reshape(-1))), K.W5)
            worst = max(worst, float(Cn[r, n] / np.mean(Cn[r])))
        print("noise alone, A = 2, P = %d, 50 seeds: largest pss_p2avg %.2f" % (P, worst))
        assert worst < 20.0


def test_cell_search_ant_refuses_before_it_looks_for_a_device():
    L = la.lib()
    n = 3 * K.W5 + K.N
    x = np.zeros((2, n), dtype=np.complex64)
    out, per = la.CellSearch(), (la.CellSearchAnt * 2)()

    def rc(nof_samples=n, ant_stride=n, nant=2, nof_prb=6, rates=la.RATES_3GPP, periods=2, force=-1, device=0, ptr=x.ctypes.data):
        cfg = la.CellSearchCfg(periods, force, 20.0)
        return L.lsn_cell_search_ant(device, ptr, 0, nof_samples, ant_stride, nant, nof_prb, rates, C.byref(cfg), C.byref(out), per, None)

    for kw in (dict(nant=0), dict(nant=3), dict(ant_stride=n - 1), dict(nof_samples=n - 1, ant_stride=n - 1), dict(periods=3), dict(nof_prb=70), dict(rates=99),
               dict(periods=17), dict(force=3), dict(ptr=None)):
        assert rc(device=99, **kw) == INVALID, kw      # (a device that does not exist: the refusal comes first)
    assert rc(device=99) == la.LSN_ERROR_NO_DEVICE
    assert rc(device=99, nant=1) == la.LSN_ERROR_NO_DEVICE and rc(device=99, periods=1, nof_samples=2 * K.W5 + K.N) == la.LSN_ERROR_NO_DEVICE
    with pytest.raises(ValueError):
        la.cell_search_ant(x[0], 6)


def test_plan_is_the_same_whichever_antennas_are_scanned():
    a = la.carrier_scan_plan(K.RATE_SCAN, nof_antennas=2, antenna=0)
    b = la.carrier_scan_plan(K.RATE_SCAN, nof_antennas=2, antenna="all")
    assert a == b and a["nof_hypotheses"] > 0
    assert la.carrier_scan_cfg(K.RATE_SCAN, antenna="all").antenna == la.SCAN_ALL_ANTENNAS


if __name__ == "__main__":
    print(sss_candidates())

"""The HIP control chain (k_pcfich, k_pdcch_llr, k_cce_power, k_viterbi, k_pbch_llr / k_pbch_viterbi) on the streams of the independent spec
transmitter (tests/spec_downlink.py): the same ground-truth checks as tests/test_spec_control_oracle.py on the product's own taps, and bit-exact
parity with the oracle on parameter points no txgen stream reaches (Ng = 1/2 among them).  Tolerances and their derivation: that file."""
import numpy as np
import pytest

import ltesniffer_amd as la
import spec_downlink as SD
from lsn_testlib import CCE_STRIDE, MAX_LOC, MAX_SIZES
from parity import compare_candidate_tables, compare_taps, run_oracle
from test_spec_control_oracle import C_ROUND, LLR_SCALE, NCASES, PORTS, _sizes, case, check_candidates, check_llrs, mib_case

pytestmark = pytest.mark.gpu

CAND = np.dtype([("bits", "<u8"), ("rnti", "<u4"), ("flags", "<u4")])


def _phy(p):
    phy = la.Phy(nof_rx_antennas=p["nof_rx"], max_batch=4)
    assert phy.setCell(p["nof_prb"], p["nof_ports"], p["cell_id"], SD.PHICH_NG[p["ng_x6"]], cp=p["cp"])
    phy.setCandidatePruning(la.Phy.PRUNE_OFF)
    return phy


def _gpu_checks(phy, p, truth):
    """the ground-truth checks on the product's taps of subframe 0 of the last batch -> (cfi, llr, candidate table)"""
    A, P, nre = p["nof_rx"], p["nof_ports"], 12 * p["nof_prb"]
    cfi = int(phy.tap(la.TAP_CFI, 0, np.uint32, 1)[0])
    assert cfi == p["cfi"], (p, cfi)
    llr = phy.tap(la.TAP_PDCCH_LLR, 0, np.float32, 6400)
    grid = phy.tap(la.TAP_GRID, 0, np.complex64, A * 14 * nre).reshape(A, 14, nre)
    ce = phy.tap(la.TAP_CE, 0, np.complex64, P * A * 14 * nre).reshape(P, A, 14, nre)
    chest = phy.tap(la.TAP_CHEST, 0, np.float32, 31 if P == 4 else 19)
    sign, mean, ratio = check_llrs(llr, truth, grid, ce, float(chest[-5]), p)   # chest[-5]: noise_avg
    assert sign == 0 and LLR_SCALE[0] <= mean <= LLR_SCALE[1] and ratio <= C_ROUND, (p, sign, mean, ratio)
    # k_cce_power: mean |LLR| of each CCE against float64; a sequential float32 sum of 72 positive terms is within 72 ulp
    ncce = truth["nof_cce"]
    pw = phy.tap(la.TAP_CCE_POWER, 0, np.float32, CCE_STRIDE)[:ncce].astype(np.float64)
    ref = np.abs(llr.astype(np.float64)).reshape(ncce, 72).mean(axis=1)
    assert np.all(np.abs(pw - ref) <= 80 * 2.0 ** -24 * ref), (p, float(np.max(np.abs(pw - ref) / ref)))
    cand = phy.tap(la.TAP_CANDIDATES, 0, np.uint8, MAX_LOC * MAX_SIZES * 16).view(CAND)
    sz = _sizes(p["nof_prb"], p["nof_ports"], p["cell_id"], p["ng_x6"], p["cp"])
    bad = check_candidates(cand, truth, p, sz)
    assert not bad, (p, bad)
    return cfi, llr, cand


def _parity(phy, p, iq):
    sc = dict(p, phich_ng_x6=p["ng_x6"])
    tti = 10 * p["sfn"] + p["sf_idx"]
    _, per_sf, _ = run_oracle(sc, tti, iq[None])
    bad = compare_taps(phy, per_sf, sc, 0, 1)
    assert not bad, (p, bad[:3])
    bad = compare_candidate_tables(phy, per_sf, sc, tti, 0, 1)
    assert not bad, (p, bad[:3])


@pytest.mark.parametrize("i", range(NCASES))
def test_gpu_control_chain_on_the_spec_transmitter(i):
    p, iq, truth = case(i)
    phy = _phy(p)
    phy.process_host(iq[None], 10 * p["sfn"] + p["sf_idx"], 0)
    _gpu_checks(phy, p, truth)
    _parity(phy, p, iq)
    phy.close()


@pytest.mark.parametrize("i", (3, 16, 29))
def test_gpu_equaliser_arithmetic_with_noise(i):
    p, iq, truth = case(i, snr_db=14.0)
    phy = _phy(p)
    phy.process_host(iq[None], 10 * p["sfn"] + p["sf_idx"], 0)
    A, P, nre = p["nof_rx"], p["nof_ports"], 12 * p["nof_prb"]
    assert int(phy.tap(la.TAP_CFI, 0, np.uint32, 1)[0]) == p["cfi"]
    llr = phy.tap(la.TAP_PDCCH_LLR, 0, np.float32, 6400)
    grid = phy.tap(la.TAP_GRID, 0, np.complex64, A * 14 * nre).reshape(A, 14, nre)
    ce = phy.tap(la.TAP_CE, 0, np.complex64, P * A * 14 * nre).reshape(P, A, 14, nre)
    noise = float(phy.tap(la.TAP_CHEST, 0, np.float32, 31 if P == 4 else 19)[-5])
    assert noise > 1e-3
    _, _, ratio = check_llrs(llr, truth, grid, ce, noise, p, noiseless=False)
    assert ratio <= C_ROUND, (p, ratio)
    _parity(phy, p, iq)
    phy.close()


def test_gpu_amplitude_sweep_keeps_cfi_candidates_and_llrs():
    """x 2^-12, x 1, x 2^12 of one stream: the kernel-edge case of reg_equalise's arithmetic"""
    out = []
    for scale in (2.0 ** -12, 1.0, 2.0 ** 12):
        p, iq, truth = case(22, scale=scale)
        phy = _phy(p)
        phy.process_host(iq[None], 10 * p["sfn"] + p["sf_idx"], 0)
        cfi, llr, cand = _gpu_checks(phy, p, truth)
        out.append((cfi, llr.copy(), cand.copy()))
        phy.close()
    for cfi, llr, cand in out[::2]:
        assert cfi == out[1][0] and np.array_equal(cand, out[1][2])
        assert np.abs(llr - out[1][1]).max() <= 1e-4


@pytest.mark.parametrize("ports", PORTS)
@pytest.mark.parametrize("q", range(4))
def test_gpu_mib_of_every_quarter_and_port_count(ports, q):
    p, iq, truth = mib_case(ports, q, q // 2)
    phy = la.Phy(nof_rx_antennas=p["nof_rx"], max_batch=4)
    assert phy.setCell(p["nof_prb"], ports, p["cell_id"], SD.PHICH_NG[p["ng_x6"]], cp=p["cp"])
    g, llr = phy.mib_decode(iq, with_llr=True)
    mib = int("".join(map(str, truth["mib"])), 2)
    assert g["found"] == 1 and (g["sfn"], g["sfn_offset"], g["nof_prb"], g["nof_ports"], g["phich_resources_x6"], g["phich_length"], g["mib_bits"]) == \
        (p["sfn"], q, p["nof_prb"], ports, p["ng_x6"], 0, mib), (p, g)
    n = len(truth["pbch_bits"])
    assert np.array_equal(llr[:n] > 0, truth["pbch_bits"] == 1) and not np.any(llr[n:])
    phy.close()

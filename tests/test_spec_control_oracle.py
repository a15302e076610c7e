"""The oracle's downlink control chain against an independent transmitter written from the specifications (tests/spec_downlink.py).

Every other control-region test loops the oracle back on tools/txgen, which shares its reading of TS 36.211 / 36.212 (and spec/lte_tables.h) with the
oracle and the product: a shared misreading passes them all.  Here the stream comes from spec_downlink.py and the checks are against its ground truth:
the CFI, the sign of every PDCCH soft bit in CCE order, their scale, the equaliser arithmetic (a float64 evaluation on the oracle's own grid and
channel estimate), every placed DCI in the candidate table with the search-space verdict of a 36.213 9.1.1 model, and the MIB.  The HIP path equals
the oracle bit for bit (tests/test_gpu_parity.py); tests/test_gpu_spec_control.py puts the same streams through it.

Tolerances (measured over the sweep below on flat, noiseless channels):
  * mean |LLR| in [0.97, 1.12]: 1.0 by construction of the scale (QPSK at +-1/sqrt2, LLR = -sqrt2 x); the 5-tap smoother of the channel
    estimate attenuates the outermost pilots (an error floor near -27 dB, tests/test_frontend_truth.py), which reads as |LLR| above 1 where the
    band edges are a large share of the REGs, and the single-port equaliser's noise term pulls it below.  Observed: 1.0012 (100 PRB, one port)
    to 1.106 (6 PRB, two ports); 0.999 to 1.102 with AWGN at 14 dB.
  * equaliser arithmetic: |llr - model| <= C_ROUND 2^-24 (M + |model|), M the sum of the magnitudes of the terms of the float32 expression divided
    by its denominator (spec_downlink.equalise); a handful of roundings per term make C = 4 ample; the largest ratio observed is 1.25 (1.08 with AWGN)."""
import ctypes as C

import numpy as np
import pytest

import spec_downlink as SD
from lsn_testlib import MAX_SIZES, OCell, OracleWorker, candidate_table, oracle
from test_pbch_oracle import oracle_mib

BWS, PORTS, CPS = (6, 15, 25, 50, 75, 100), (1, 2, 4), (0, 1)
NGS = (1, 3, 6, 12)             # 6 Ng: 1/6, 1/2, 1, 2
C_ROUND = 4.0
LLR_SCALE = (0.97, 1.12)
# cell IDs: 0 and 503, every id mod 3, and (with the bandwidths they meet) N_ID mod 2 N_RB >= N_RB, where the PCFICH REGs wrap past the band
CIDS = (0, 503, 301, 77, 150, 11, 34, 262, 5, 419, 88, 196)


def _sizes(nprb, ports, cid, ng, cp):
    cell = OCell(nprb, ports, cid, ng, 0, cp)
    return sorted({oracle().o_dci_format_sizeof(C.byref(cell), f) for f in range(9)})


def _rnti_for(nof_cce, L, n, sf_idx, rng):
    """a C-RNTI whose UE-specific space holds (L, n), or None"""
    for _ in range(4000):
        r = int(rng.integers(0x000B, 0xFFF4))
        if (L, n) in SD.search_space(nof_cce, r, sf_idx) and SD.validate_location(nof_cce, n, L, sf_idx, r) == 2:
            return r
    return None


def case(i, snr_db=None, scale=1.0):
    """case i of the covering design: every bandwidth x port count x prefix once; rx, Ng, CFI, cell ID and subframe rotated across them"""
    nprb, ports, cp = BWS[i // 6], PORTS[(i // 2) % 3], CPS[i % 2]
    p = dict(nof_prb=nprb, nof_ports=ports, cp=cp, nof_rx=1 + (i // 2 + i // 6) % 2, ng_x6=NGS[(i + i // 6) % 4], cfi=1 + (i + i // 4 + 1) % 3,
             cell_id=CIDS[i % len(CIDS)], sf_idx=i % 10, sfn=4 * 173 + i % 4)
    rng = np.random.default_rng(1000 + i)
    reg = SD.ControlRegion(nprb, ports, p["cell_id"], cp, p["ng_x6"])
    ncce = reg.nof_cce(p["cfi"])
    lim = min(ncce, 84)              # the candidate table covers the first 84 CCEs
    sz = _sizes(nprb, ports, p["cell_id"], p["ng_x6"], cp)
    taken = np.zeros(ncce, dtype=bool)
    dcis = []
    # an SI-RNTI DCI in the common space (L = 4 or 8 at CCE 0), then one DCI per level where it fits, the smallest and largest sizes first
    plan = [(8, SD.SI_RNTI), (4, SD.SI_RNTI)] if i % 3 == 0 else []
    plan += [(L, None) for L in (8, 4, 2, 1)]
    for L, rnti in plan:
        free = [n for n in range(0, lim - L + 1, L) if not taken[n:n + L].any()]
        if not free or (rnti == SD.SI_RNTI and (0 not in free or any(d[2] == SD.SI_RNTI for d in dcis))):
            continue
        n = 0 if rnti == SD.SI_RNTI else free[int(rng.integers(len(free)))]
        if rnti is None:
            rnti = _rnti_for(ncce, L, n, p["sf_idx"], rng) if len(dcis) % 2 == 0 else int(rng.integers(0x000B, 0xFFF4))
            if rnti is None:
                rnti = int(rng.integers(0x000B, 0xFFF4))
        nb = (sz[0], sz[-1])[len(dcis)] if len(dcis) < 2 else sz[int(rng.integers(len(sz)))]
        taken[n:n + L] = True
        dcis.append((L, n, rnti, rng.integers(0, 2, nb).astype(np.uint8)))
    iq, truth = SD.control_subframe(dcis=dcis, seed=i, snr_db=snr_db, scale=scale, **p)
    return p, iq, truth


NCASES = len(BWS) * len(PORTS) * len(CPS)
NOISY = (3, 16, 29)   # + AWGN at 14 dB: the equaliser check with noise_avg != 0


def run_case(p, iq):
    ow = OracleWorker(p["nof_prb"], p["nof_ports"], p["cell_id"], p["nof_rx"], p["ng_x6"], cp=p["cp"])
    ow.work(iq, 10 * p["sfn"] + p["sf_idx"])
    return ow


def candidate_row(L, n, nof_cce):
    """row of location (L, first CCE n) in the candidate table (lsn_testlib.candidate_table: levels 8, 4, 2, 1, each over the first 84 CCEs)"""
    lim, row = min(nof_cce, 84), 0
    for LL in (8, 4, 2, 1):
        if LL == L:
            assert n // L < lim // L
            return row + n // L
        row += lim // LL


def check_candidates(cand, truth, p, sz):
    """every placed DCI at its (L, ncce) row and its size column: payload, RNTI and the search-space model's verdict"""
    bad = []
    for L, n, rnti, payload in truth["dcis"]:
        e = cand[candidate_row(L, n, truth["nof_cce"]) * MAX_SIZES + sz.index(len(payload))]
        bits = sum(int(b) << (63 - k) for k, b in enumerate(payload))
        want = 1 | (SD.validate_location(truth["nof_cce"], n, L, p["sf_idx"], rnti) << 1)
        if (int(e["bits"]), int(e["rnti"]), int(e["flags"])) != (bits, rnti, want):
            bad.append((L, n, hex(rnti), len(payload), hex(int(e["bits"])), hex(bits), hex(int(e["rnti"])), int(e["flags"]), want))
    return bad


def check_llrs(llr, truth, grid, ce, noise, p, noiseless=True):
    """-> (sign errors, mean |LLR|, largest |llr - model| / its rounding bound)"""
    n = 72 * truth["nof_cce"]
    assert len(llr) == n, (len(llr), n)
    model, mag = SD.pdcch_llr_model(grid, ce, noise, truth["reg"], truth["cfi"], p["sf_idx"])
    ratio = float(np.max(np.abs(model - llr.astype(np.float64)) / (2.0 ** -24 * (mag + np.abs(model)))))
    sign = int(np.sum((llr > 0) != (truth["pdcch_bits"] == 1))) if noiseless else 0
    return sign, float(np.mean(np.abs(llr.astype(np.float64)))), ratio


def test_covering_design_reaches_every_parameter():
    ps = [case(i)[0] for i in range(NCASES)]
    assert {(p["nof_prb"], p["nof_ports"], p["cp"]) for p in ps} == {(b, q, c) for b in BWS for q in PORTS for c in CPS}
    assert {p["nof_rx"] for p in ps} == {1, 2} and {p["ng_x6"] for p in ps} == set(NGS) and {p["cfi"] for p in ps} == {1, 2, 3}
    assert {p["sf_idx"] for p in ps} == set(range(10)) and {p["cell_id"] % 3 for p in ps} == {0, 1, 2}
    assert {0, 503} <= {p["cell_id"] for p in ps}
    assert any(p["cell_id"] % (2 * p["nof_prb"]) >= p["nof_prb"] for p in ps)
    assert any(p["nof_prb"] <= 10 and p["cp"] and p["cfi"] == 3 for p in ps)   # four control symbols, the fourth with 6-RE REGs (36.211 6.2.4)


def test_placed_dcis_cover_every_level_both_size_extremes_and_si_rnti():
    seen = set()
    for i in range(NCASES):
        p, _, truth = case(i)
        sz = _sizes(p["nof_prb"], p["nof_ports"], p["cell_id"], p["ng_x6"], p["cp"])
        for L, n, rnti, payload in truth["dcis"]:
            seen |= {("L", L), ("size", len(payload) == sz[0], len(payload) == sz[-1])}
            if rnti == SD.SI_RNTI:
                seen.add("si")
            seen.add(("verdict", SD.validate_location(truth["nof_cce"], n, L, p["sf_idx"], rnti)))
    assert {("L", L) for L in (1, 2, 4, 8)} <= seen and "si" in seen
    assert any(s[:2] == ("size", True) for s in seen if s[0] == "size") and any(s[2] for s in seen if s[0] == "size")
    assert {("verdict", v) for v in (0, 2)} <= seen


def test_spec_model_known_answers():
    """hand-checkable points of the model itself: the CRC of 36.212 5.1.1 on a one-bit message is the polynomial, the generator taps, the
    interleaver is a permutation, and the PHICH of Ng = 1/2 at 25 PRB takes ceil(0.5 * 25 / 8) = 2 groups = 6 REGs"""
    assert SD.crc16([1]) == [int(c) for c in format(SD.G_CRC16 & 0xFFFF, "016b")]
    d = SD.conv_encode([1] + [0] * 9)  # the impulse response of each generator: c_k-j taps, k = j
    assert [int("".join(map(str, d[s, :7])), 2) for s in range(3)] == [0o133, 0o171, 0o165]
    assert sorted(q for q in SD.subblock_cc(100) if q >= 0) == list(range(100))
    assert len(SD.ControlRegion(25, 2, 7, 0, 3).phich) == 6 and SD.ControlRegion(25, 2, 7, 1, 3).ngroup == 4
    assert SD.ControlRegion(6, 1, 0, 1, 1).nof_symbols(3) == 4


@pytest.mark.parametrize("i", range(NCASES))
def test_control_chain_on_the_spec_transmitter(i):
    p, iq, truth = case(i)
    ow = run_case(p, iq)
    assert ow.cfi() == p["cfi"], (p, ow.cfi())
    sign, mean, ratio = check_llrs(ow.llr(), truth, ow.grid(), ow.ce(), ow.chest().noise_avg, p)
    assert sign == 0, (p, sign)
    assert LLR_SCALE[0] <= mean <= LLR_SCALE[1], (p, mean)
    assert ratio <= C_ROUND, (p, ratio)
    sz = _sizes(p["nof_prb"], p["nof_ports"], p["cell_id"], p["ng_x6"], p["cp"])
    cand, _ = candidate_table(ow.llr(), truth["nof_cce"], sz, p["sf_idx"])
    cand = np.frombuffer(bytes(cand), dtype=np.dtype([("bits", "<u8"), ("rnti", "<u4"), ("flags", "<u4")]))
    bad = check_candidates(cand, truth, p, sz)
    assert not bad, (p, bad)


@pytest.mark.parametrize("i", NOISY)
def test_equaliser_arithmetic_with_noise(i):
    p, iq, truth = case(i, snr_db=14.0)
    ow = run_case(p, iq)
    assert ow.cfi() == p["cfi"] and ow.chest().noise_avg > 1e-3
    _, _, ratio = check_llrs(ow.llr(), truth, ow.grid(), ow.ce(), ow.chest().noise_avg, p, noiseless=False)
    assert ratio <= C_ROUND, (p, ratio)
    sz = _sizes(p["nof_prb"], p["nof_ports"], p["cell_id"], p["ng_x6"], p["cp"])
    cand, _ = candidate_table(ow.llr(), truth["nof_cce"], sz, p["sf_idx"])
    cand = np.frombuffer(bytes(cand), dtype=np.dtype([("bits", "<u8"), ("rnti", "<u4"), ("flags", "<u4")]))
    assert not check_candidates(cand, truth, dict(p), sz)


@pytest.mark.parametrize("scale", [2.0 ** -12, 2.0 ** 12])
def test_amplitude_does_not_move_cfi_candidates_or_llrs(scale):
    i = 22
    p, iq, truth = case(i, scale=scale)
    ow = run_case(p, iq)
    assert ow.cfi() == p["cfi"]
    sign, mean, ratio = check_llrs(ow.llr(), truth, ow.grid(), ow.ce(), ow.chest().noise_avg, p)
    assert sign == 0 and LLR_SCALE[0] <= mean <= LLR_SCALE[1] and ratio <= C_ROUND, (sign, mean, ratio)
    _, iq1, _ = case(i)
    ow1 = run_case(p, iq1)
    assert np.abs(ow.llr() - ow1.llr()).max() <= 1e-4


def mib_case(ports, q, cp):
    nprb = BWS[(3 * ports + q) % 6]
    p = dict(nof_prb=nprb, nof_ports=ports, cp=cp, nof_rx=1 + q % 2, ng_x6=NGS[(q + ports) % 4], cfi=1 + q % 3, cell_id=CIDS[(q + 5 * ports) % len(CIDS)],
             sf_idx=0, sfn=4 * (17 + 41 * ports) + q)
    iq, truth = SD.control_subframe(seed=q + 10 * ports, **p)
    return p, iq, truth


@pytest.mark.parametrize("ports", PORTS)
@pytest.mark.parametrize("q", range(4))
def test_mib_of_every_quarter_and_port_count(ports, q):
    p, iq, truth = mib_case(ports, q, q // 2)
    sc = dict(p, phich_ng_x6=p["ng_x6"])
    r, m = oracle_mib(sc, iq)
    mib = int("".join(map(str, truth["mib"])), 2)
    assert r == 1 and m.found and (m.sfn, m.sfn_offset, m.nof_prb, m.nof_ports, m.phich_ng_x6, m.phich_length, m.mib_bits) == \
        (p["sfn"], q, p["nof_prb"], ports, p["ng_x6"], 0, mib), (p, m.sfn, m.sfn_offset, m.nof_prb, m.nof_ports, m.phich_ng_x6)
    llr = np.zeros(480, dtype=np.float32)
    oracle_mib(sc, iq, llr)
    n = len(truth["pbch_bits"])
    assert np.array_equal(llr[:n] > 0, truth["pbch_bits"] == 1)

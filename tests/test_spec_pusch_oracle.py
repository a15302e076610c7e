"""The oracle's PUSCH chain (SC-FDMA demodulation, reference-signal channel estimate, equaliser, transform de-precoding, soft demodulation,
descrambling, channel de-interleaver with the control-information layout, rate de-matching, turbo decoder) against an independent transmitter written
from the specifications (tests/spec_uplink.py; the DCI format 0 of tests/spec_dci.py).

Every other test of the uplink loops the oracle back on tools/txgen, which shares its reading of TS 36.211 / 36.212 / 36.213 with the oracle and the
product.  Here the truth is what the spec transmitter sent and every check is exact: (a) the CRC passes and the payload is the transmitted one; (b) the
number of soft bits is G, every soft bit has the sign of the transmitted UL-SCH bit and is not zero - except exactly the positions a HARQ-ACK symbol
overwrote, which are exactly 0; (c) K / F / E / rv of every code block equal the independent segmentation and the de-rate-matched streams have the
encoder's signs where the redundancy version covers a position and are 0 where it does not; (d) with the RNTI or the cyclic-shift field off by one
the block does not decode.  tests/test_gpu_spec_pusch.py puts the same streams through the HIP kernels.

Conditions on the inputs (not exemptions in a check): noise-free cases carry a random gain of +-3 dB and a random phase; a delay of 1 - 2 samples only
in QPSK / 16QAM cases - the receiver's three-tap smoother of the channel estimate has two taps at the allocation edge and is biased on a phase ramp,
which the dense constellations do not survive at the edge carriers.

One departure of the receiver from the letter of 36.213 8.4.1, reference behaviour (ul_sniffer_pusch.c:58), is asserted exactly in
test_type1_hopping_offset_against_the_letter_of_the_specification (HOP_DEPARTS).

Q' known answers, by hand (5.2.2.6, Q' = min(ceil(O M_sc N_symb beta / sum K), cap)):
  * 6 PRB, normal CP, TBS 1032 (one block, K = 1056), defaults beta_RI = 15.875, beta_CQI = 2.25: one RI bit: 72 x 12 x 15.875 / 1056 = 12.99 -> 13; an 18-bit
    report (O > 11: 8 CRC bits more, 26): 26 x 72 x 12 x 2.25 / 1056 = 47.86 -> 48.
  * 1 PRB, TBS 16 (K = 40), one HARQ-ACK bit, beta = 20: 12 x 12 x 20 / 40 = 72 -> the cap 4 M_sc = 48.
  * 3 PRB, extended CP (N_symb = 10), TBS 208 (K = 232): HARQ-ACK 36 x 10 x 20 / 232 = 31.03 -> 32; RI 360 x 15.875 / 232 = 24.6 -> 25; CQI 26 x 360 x 2.25 / 232 = 90.8 -> 91.
  * 5 PRB, TBS 2216 (K = 2240), two HARQ-ACK bits: 2 x 60 x 12 x 20 / 2240 = 12.86 -> 13.

AWGN cases (a condition on the inputs, not a tolerance): NOISY_SNR_DB = 26 dB on cases NOISY; noise variance 10^(-2.6) per resource element against a
grant of unit gain (the cases keep their gain of +-3 dB).  Swept on the CPU oracle in 1 dB steps from 30 dB down with the seeds of the cases: the first
payload is lost at 18 dB (case 5: 64QAM at rate 0.85, three blocks), 20 dB (case 6: 256QAM, extended CP) and 14 dB (case 14: 64QAM under two HARQ-ACK bits);
every step above decodes.  26 dB is 6 dB above the first failure of the weakest case.  At that SNR (a) and the segmentation and block CRCs of (c) are
asserted; the signs of single soft bits are what noise turns."""
import ctypes as C
import functools

import numpy as np
import pytest

import spec_dci as DCI
import spec_pdsch as SP
import spec_uplink as SU
from lsn_testlib import OCell, OPuschGrant, OUci, OUlCfg, oracle_trace, oracle_trace_enable, oracle_ul_api, pusch_hop_slot1
from test_spec_pdsch_oracle import check_d3
from test_spec_tables import _arr

# One subframe per case.  cs: cyclicShift of SIB2, dss: groupAssignmentPUSCH, gh / sh: group / sequence hopping, ho: pusch-HoppingOffset;
# grants: n (first PRB), L, mcs (36.213 Table 8.6.1-1), nd: the cyclic shift field of DCI format 0; optional rv, qm (8: a 256QAM transmission of the same
# block), delay (samples), hop: the hopping bits of a type-1 grant, ack / ri / cqi: bits of control information, ia / ir / ic: beta indices
CASES = [
    dict(prb=6, cp=0, cid=300, sf=0, cs=0, dss=0, grants=[dict(n=0, L=1, mcs=4, nd=0, delay=1)]),                        # 0: one PRB at PRB 0 (tabulated sequence), QPSK
    dict(prb=6, cp=1, cid=301, sf=5, cs=1, dss=7, grants=[dict(n=4, L=2, mcs=12, nd=1, delay=2)]),                       # 1: two PRB at the top of the band, extended CP, 16QAM
    dict(prb=15, cp=0, cid=152, sf=1, cs=2, dss=0, gh=1, grants=[dict(n=6, L=3, mcs=22, nd=2)]),                         # 2: group hopping; across the centre of an odd band, 64QAM
    dict(prb=15, cp=0, cid=34, sf=2, cs=3, dss=29, sh=1, grants=[dict(n=10, L=5, mcs=8, nd=3, delay=1)]),                # 3: sequence hopping below 6 PRB: no effect
    dict(prb=25, cp=0, cid=447, sf=3, cs=4, dss=0, sh=1, grants=[dict(n=9, L=6, mcs=16, nd=4)]),                         # 4: sequence hopping at 6 PRB: v = 1
    dict(prb=25, cp=0, cid=100, sf=4, cs=5, dss=3, grants=[dict(n=0, L=25, mcs=28, nd=5)]),                              # 5: full band, 64QAM at rate 0.85, three blocks
    dict(prb=25, cp=1, cid=503, sf=6, cs=6, dss=0, grants=[dict(n=11, L=3, mcs=24, nd=6, qm=8)]),                        # 6: 256QAM, extended CP
    dict(prb=15, cp=0, cid=11, sf=7, cs=7, dss=0, grants=[dict(n=13, L=2, mcs=2, nd=7, rv=2, delay=2)]),                 # 7 - 9: rv 2, 3, 1, each decoded alone
    dict(prb=6, cp=0, cid=88, sf=8, cs=0, dss=12, grants=[dict(n=2, L=3, mcs=1, nd=3, rv=3)]),
    dict(prb=25, cp=1, cid=262, sf=9, cs=2, dss=0, grants=[dict(n=20, L=5, mcs=3, nd=5, rv=1, delay=1)]),
    dict(prb=100, cp=0, cid=77, sf=2, cs=3, dss=0, grants=[dict(n=0, L=100, mcs=28, nd=1)]),                             # 10: 100 PRB: M_sc = 1200, 13 code blocks
    dict(prb=25, cp=0, cid=196, sf=1, cs=1, dss=0, ho=2, grants=[dict(n=3, L=3, mcs=9, nd=2, hop=0)]),                   # 11: type-1 hopping, one hopping bit
    dict(prb=50, cp=0, cid=419, sf=6, cs=5, dss=0, ho=4, grants=[dict(n=20, L=6, mcs=15, nd=4, hop=1)]),                 # 12: type-1 hopping, two hopping bits (-1/4)
    dict(prb=15, cp=0, cid=5, sf=3, cs=6, dss=0, grants=[dict(n=0, L=3, mcs=13, nd=0, ack=1)]),                          # 13: one HARQ-ACK bit
    dict(prb=25, cp=0, cid=150, sf=0, cs=7, dss=0, grants=[dict(n=12, L=5, mcs=22, nd=6, ack=2)]),                       # 14: two HARQ-ACK bits, 64QAM
    dict(prb=25, cp=0, cid=301, sf=4, cs=4, dss=0, grants=[dict(n=19, L=6, mcs=10, nd=7, ri=1, cqi=18, delay=1)]),       # 15: RI + the 4 + 2 N-bit CQI report (N = ceil(25 / 4))
    dict(prb=25, cp=0, cid=34, sf=8, cs=2, dss=0, grants=[dict(n=3, L=5, mcs=6, nd=1, ack=1, ri=1, cqi=18)]),            # 16: all three
    dict(prb=25, cp=0, cid=88, sf=5, cs=0, dss=0, grants=[dict(n=10, L=6, mcs=14, nd=2, ack=2, ri=1, cqi=18, ia=7, ir=5, ic=12)]),   # 17: the UE's own beta offsets
    dict(prb=25, cp=1, cid=11, sf=7, cs=3, dss=0, grants=[dict(n=22, L=3, mcs=5, nd=0, ack=1, ri=1, cqi=18)]),           # 18: control information under the extended CP
    dict(prb=6, cp=0, cid=447, sf=9, cs=1, dss=0, grants=[dict(n=5, L=1, mcs=0, nd=4, ack=1)]),                          # 19: Q'_ACK at its cap 4 M_sc
    dict(prb=15, cp=0, cid=262, sf=6, cs=5, dss=21, grants=[dict(n=4, L=3, mcs=13, nd=3, delay=1), dict(n=7, L=2, mcs=5, nd=6), dict(n=9, L=1, mcs=17, nd=7)]),   # 20: neighbours
]
NCASES = len(CASES)
NOISY = (5, 6, 14)
# swept on the CPU oracle in 1 dB steps from 30 dB down, with the seeds of the cases: the payload is first lost at SWEPT[case] dB - case 5 (64QAM at rate 0.85,
# 25 PRB, three blocks) at 18 dB, case 6 (256QAM at rate 0.52, 3 PRB, extended CP) at 20 dB, case 14 (64QAM at rate 0.52 under two HARQ-ACK bits) at 14 dB; every
# step above decodes.  NOISY_SNR_DB is 6 dB above the first failure of the weakest case.
SWEPT = {5: 18, 6: 20, 14: 14}
NOISY_SNR_DB = max(SWEPT.values()) + 6.0


def _cell(c):
    return dict(nof_prb=c["prb"], cell_id=c["cid"], cp=c["cp"], cyclic_shift=c["cs"], delta_ss=c["dss"], group_hopping=c.get("gh", 0), sequence_hopping=c.get("sh", 0),
                hopping_offset=c.get("ho", 0))


@functools.lru_cache(maxsize=None)
def case(i, snr_db=None):
    """-> (cell, sf_idx, iq[15 N], truth per grant); the grant dicts (truth[k]["grant"]) carry what a receiver is told: rnti, n_prb, L_prb, mod, tbs, rv, n_dmrs, ..."""
    c = CASES[i]
    cell = _cell(c)
    rng = np.random.default_rng(9000 + i)
    grants = []
    for s in c["grants"]:
        qm, tbs = SU.tbs_of(s["mcs"], s["L"], s.get("qm"))
        g = dict(rnti=int(rng.integers(0x000B, 0xFFF3)), n_prb=s["n"], L_prb=s["L"], mod=qm, tbs=tbs, rv=s.get("rv", 0), n_dmrs=s["nd"], delay=s.get("delay", 0),
                 nof_ack=s.get("ack", 0), ri_bits=s.get("ri", 0), cqi_bits=s.get("cqi", 0))
        g.update({k: s[j] for j, k in (("ia", "i_ack"), ("ir", "i_ri"), ("ic", "i_cqi")) if j in s})
        if "hop" in s:
            g.update(hop=1, n_prb2=pusch_hop_slot1(c["prb"], c["ho"], s["hop"], s["n"]))
        grants.append(g)
    iq, truths = SU.subframe(cell, c["sf"], grants, seed=i, snr_db=snr_db)
    return cell, c["sf"], iq, truths


# ---------------------------------------------------------------------------------------------------------------------------- checks shared with the GPU file (arrays in, no oracle handles)
def check_grant(res, t, noisy=False):
    """res: dict(crc_ok, payload, llr int16[], cbs: list of dict(K, F, E, rv, ok, d3)) of one grant; t: the transmitter's truth.  Checks (a), (b), (c)"""
    assert res["crc_ok"] == 1 and res["payload"] == t["payload"], ("(a) payload", res["crc_ok"])
    llr = np.asarray(res["llr"], dtype=np.int64)
    assert len(llr) == t["G"], ("(b) number of soft bits", len(llr), t["G"])
    p = t["punct"]
    if not noisy:
        assert np.count_nonzero(p) == t["Qm"] * np.count_nonzero((t["kind"] == SU.ACK) & (t["gidx"] >= t["q_cqi"]))
        assert not np.any(llr[p]), ("(b) a HARQ-ACK position is not 0", int(np.count_nonzero(llr[p])))
        zero = (llr == 0) & ~p
        wrong = (llr != 0) & ((llr > 0) != (t["f"] == 1)) & ~p       # positive = bit 1 (o_pusch.c, demod_llr)
        assert not zero.any(), ("(b) zero soft bits", int(zero.sum()), np.nonzero(zero)[0][:8])
        assert not wrong.any(), ("(b) soft-bit signs", int(wrong.sum()), np.nonzero(wrong)[0][:8])
    cbs = res["cbs"]
    assert len(cbs) == t["seg"]["C"] == len(t["blocks"]), (len(cbs), t["seg"]["C"])
    o = 0
    for r, (cb, b) in enumerate(zip(cbs, t["blocks"])):
        assert (cb["K"], cb["F"], cb["E"], cb["rv"]) == (b["K"], b["F"], b["E"], t["rv"]), ("(c)", r, cb["K"], cb["F"], cb["E"], cb["rv"], b["K"], b["F"], b["E"], t["rv"])
        if not noisy:
            check_d3(cb["d3"], b, p[o:o + b["E"]])
        o += b["E"]
        assert cb["ok"] == 1, ("(c) block CRC", r)
    assert o == t["G"]
    return len(cbs), len(llr)


def receiver_grant(t, rnti_xor=0, nd_add=0):
    """what the receiver is told about a grant (the format of Phy.pusch_decode), optionally with the RNTI / the cyclic-shift field off by one"""
    g = t["grant"]
    out = dict(sf=0, rnti=g["rnti"] ^ rnti_xor, n_dmrs=(g["n_dmrs"] + nd_add) % 8, n_prb=g["n_prb"], L_prb=g["L_prb"], mod=g["mod"], tbs=g["tbs"], rv=g["rv"],
               nof_ack=g["nof_ack"], cqi_bits=g["cqi_bits"], ri_bits=g["ri_bits"], hop=g.get("hop", 0), n_prb2=g.get("n_prb2", 0))
    out.update({k + "_p1": g[k] + 1 for k in ("i_ack", "i_cqi", "i_ri") if k in g})
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the oracle on one subframe
def _api():
    o = oracle_ul_api()
    o.o_uci_layout_cp.argtypes = [C.c_int, C.c_int, C.POINTER(OUci), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    o.o_trace_begin_job.argtypes = [C.c_uint32, C.c_uint16, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    o.o_trace_begin_job.restype = None
    return o


def oracle_structs(cell):
    return (OCell(cell["nof_prb"], 1, cell["cell_id"], 1, cell["hopping_offset"], cell["cp"]),
            OUlCfg(cell["cyclic_shift"], cell["delta_ss"], cell["hopping_offset"], cell["group_hopping"], cell["sequence_hopping"]))


def oracle_grid(cell, iq):
    ocell, _ = oracle_structs(cell)
    grid = np.zeros(14 * 12 * cell["nof_prb"], dtype=np.complex64)
    _api().o_ul_fft(C.byref(ocell), np.ascontiguousarray(iq).ctypes.data, grid.ctypes.data)
    return grid


def oracle_grant(cell, sf_idx, grid, rg, max_iter=12):
    """one grant (receiver_grant format) through o_pusch_demod_uci and o_pusch_decode_uci -> dict(crc_ok, payload, llr, cbs, iterations, snr_db, q: (Q'_ACK, Q'_RI, Q'_CQI))"""
    o = _api()
    ocell, ucfg = oracle_structs(cell)
    og = OPuschGrant(rg["L_prb"], rg["n_prb"], 0, rg["mod"], rg["tbs"], rg["rv"], rg["n_prb2"], rg["hop"])
    uci = OUci(rg["nof_ack"], rg["cqi_bits"], rg["ri_bits"], rg.get("i_ack_p1", 0), rg.get("i_cqi_p1", 0), rg.get("i_ri_p1", 0))
    M = 12 * rg["L_prb"]
    cls, didx = np.zeros(12 * M, np.uint8), np.zeros(12 * M, np.int32)
    qa, qr, qc = C.c_int(), C.c_int(), C.c_int()
    nsym = o.o_uci_layout_cp(M, rg["tbs"], C.byref(uci), cell["cp"], cls.ctypes.data, didx.ctypes.data, C.byref(qa), C.byref(qr), C.byref(qc))
    assert nsym > 0
    G = nsym * rg["mod"]
    e = np.zeros(12 * M * rg["mod"], dtype=np.int16)
    assert o.o_pusch_demod_uci(C.byref(ocell), C.byref(ucfg), sf_idx, rg["rnti"], C.byref(og), rg["n_dmrs"], C.byref(uci), grid.ctypes.data, e.ctypes.data, None, None) == 0
    out = np.zeros(rg["tbs"] // 8 + 8, dtype=np.uint8)
    its, snr = C.c_int(0), C.c_float(0)
    oracle_trace_enable(True)
    o.o_trace_begin_job(sf_idx, rg["rnti"], 0, None, None, None, 1)
    crc = o.o_pusch_decode_uci(C.byref(ocell), C.byref(ucfg), sf_idx, rg["rnti"], C.byref(og), rg["n_dmrs"], C.byref(uci), grid.ctypes.data, max_iter, out.ctypes.data,
                               C.byref(its), C.byref(snr))
    cbs = oracle_trace()[0]["cbs"]
    oracle_trace_enable(False)
    return dict(crc_ok=crc, payload=bytes(out[:rg["tbs"] // 8]) if crc else b"", llr=e[:G].copy(), cbs=cbs, iterations=its.value, snr_db=snr.value,
                q=(qa.value, qr.value, qc.value))


def _run_case(i, snr_db=None):
    cell, sf, iq, truths = case(i, snr_db)
    grid = oracle_grid(cell, iq)
    n = 0
    for t in truths:
        res = oracle_grant(cell, sf, grid, receiver_grant(t))
        assert res["q"] == (t["q_ack"], t["q_ri"], t["q_cqi"]), ("Q'", res["q"], t["q_ack"], t["q_ri"], t["q_cqi"])
        ncb, nllr = check_grant(res, t, noisy=snr_db is not None)
        assert ncb == t["seg"]["C"] and nllr == t["G"]
        n += 1
    assert n == len(CASES[i]["grants"])
    return cell, sf, grid, truths


@pytest.mark.parametrize("i", range(NCASES))
def test_pusch_chain_on_the_spec_transmitter(i):
    cell, sf, grid, truths = _run_case(i)
    for t in truths:    # (d)
        assert oracle_grant(cell, sf, grid, receiver_grant(t, rnti_xor=1), max_iter=4)["crc_ok"] == 0
        assert oracle_grant(cell, sf, grid, receiver_grant(t, nd_add=1), max_iter=4)["crc_ok"] == 0


@pytest.mark.parametrize("i", NOISY)
def test_payloads_survive_awgn(i):
    _run_case(i, NOISY_SNR_DB)


# ---------------------------------------------------------------------------------------------------------------------------- UL_MODE from a spec DCI format 0
# Six subframes, two antennas: the downlink antenna carries a DCI format 0 (spec_dci.pack_0 in spec_downlink.control_subframe) in subframe t = 1 of the stream, the
# uplink antenna the matching PUSCH in subframe t + 4 (36.213 8.0, FDD).  Pins end to end: the cyclic shift field -> n_DMRS^(2), MCS -> (Q_m, TBS, rv),
# CQI request -> the control-information layout (the 4 + 2 N-bit report and one RI bit with the default offsets), hopping flag and bits -> slot 1, and the timing.
UL_STREAMS = [
    dict(cid=77, sfn=511, sf0=7, cs=3, dss=5, ho=0, start=4, L=4, mcs=14, nd=5, cqi_request=0, hop=None),      # (i) a plain grant, 16QAM, across a frame boundary
    dict(cid=262, sfn=90, sf0=2, cs=6, dss=11, ho=0, start=15, L=6, mcs=12, nd=2, cqi_request=1, hop=None),    # (ii) CQI request: report + RI multiplexed
    dict(cid=150, sfn=1022, sf0=4, cs=1, dss=0, ho=4, start=5, L=3, mcs=13, nd=7, cqi_request=0, hop=0),       # (iii) hopping flag, pusch-HoppingOffset 4
]
UL_STREAM_CELL = dict(nof_prb=25, nof_ports=1, cp=0, cfi=3, ng_x6=1)
UL_STREAM_LEN, UL_STREAM_T = 6, 1


@functools.lru_cache(maxsize=None)
def ul_stream(k):
    """-> (sc: cell and uplink configuration, tti0, iq[6, 2, 15 N] complex64, want: [(rnti, tti, payload bytes)])"""
    import spec_downlink as SD
    from test_spec_control_oracle import _rnti_for
    s = UL_STREAMS[k]
    p = UL_STREAM_CELL
    rng = np.random.default_rng(9500 + k)
    tti0 = 10 * s["sfn"] + s["sf0"]
    reg = SD.ControlRegion(p["nof_prb"], p["nof_ports"], s["cid"], p["cp"], p["ng_x6"])
    ncce = reg.nof_cce(p["cfi"])
    sf_t = (tti0 + UL_STREAM_T) % 10
    # a new C-RNTI at level 8 on a location that is valid for it: FALCON's shortcut rule activates it at first sight
    L, n, rnti = next((L, n, r) for L in (8, 4) for n in range(0, ncce - L + 1, L) for r in [_rnti_for(ncce, L, n, sf_t, rng)] if r is not None)
    bits = DCI.pack_0(p["nof_prb"], s["start"], s["L"], s["mcs"], ndi=k % 2, tpc=k % 4, cyclic_shift=s["nd"], cqi_request=s["cqi_request"], hop=s["hop"])
    N = SU.FFT[p["nof_prb"]]
    iq = np.zeros((UL_STREAM_LEN, 2, 15 * N), dtype=np.complex64)
    for j in range(UL_STREAM_LEN):
        tti = (tti0 + j) % 10240
        dl, _ = SD.control_subframe(p["nof_prb"], p["nof_ports"], s["cid"], p["cp"], tti % 10, tti // 10, p["cfi"], p["ng_x6"], 1,
                                    dcis=[(L, n, rnti, np.array(bits, dtype=np.uint8))] if j == UL_STREAM_T else (), seed=100 * k + j)
        iq[j, 0] = dl[0]
    cell = dict(nof_prb=p["nof_prb"], cell_id=s["cid"], cp=p["cp"], cyclic_shift=s["cs"], delta_ss=s["dss"], group_hopping=0, sequence_hopping=0, hopping_offset=s["ho"])
    qm, tbs = SU.tbs_of(s["mcs"], s["L"])
    g = dict(rnti=rnti, n_prb=s["start"], L_prb=s["L"], mod=qm, tbs=tbs, rv=0, n_dmrs=s["nd"])
    if s["cqi_request"]:
        g.update(ri_bits=1, cqi_bits=4 + 2 * -(-p["nof_prb"] // 4))     # the higher-layer sub-band report the receiver assumes: sub-bands of 4 PRB on 25 PRB
    if s["hop"] is not None:
        g.update(hop=1, n_prb2=pusch_hop_slot1(p["nof_prb"], s["ho"], s["hop"], s["start"]))
        assert g["n_prb2"] == SU.hop_slot1_spec(p["nof_prb"], s["ho"], s["hop"], s["start"]) != s["start"]
    tti_ul = (tti0 + UL_STREAM_T + 4) % 10240
    ul, truths = SU.subframe(cell, tti_ul % 10, [g], seed=50 + k)
    iq[UL_STREAM_T + 4, 1] = ul
    sc = dict(p, cell_id=s["cid"], cyclic_shift=s["cs"], delta_ss=s["dss"], hopping_offset=s["ho"])
    return sc, tti0, iq, [(rnti, tti_ul, truths[0]["payload"])]


def check_ul_records(recs, want):
    """exactly one uplink MAC-LTE record, and it is the transmitted transport block: same RNTI, TTI and bytes"""
    ul = [(r["rnti"], 10 * r["sfn"] + r["sf"], r["pdu"]) for r in recs if r["direction"] == 0]
    assert len(ul) == 1, ("uplink records", [(hex(a), b, len(c)) for a, b, c in ul])
    assert ul == want, ("uplink record", hex(ul[0][0]), ul[0][1], len(ul[0][2]), hex(want[0][0]), want[0][1], len(want[0][2]))


def run_oracle_ul_stream(k):
    from lsn_testlib import OracleWorkerUl, parse_pcap
    sc, tti0, iq, want = ul_stream(k)
    ow = OracleWorkerUl(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], sc["cyclic_shift"], sc["delta_ss"], sc["hopping_offset"], cp=sc["cp"])
    for j in range(iq.shape[0]):
        ow.work_ul(iq[j, 0], iq[j, 1], (tti0 + j) % 10240, update_meta=1 if j == 0 else 0)
    return ow, parse_pcap(ow.pcap_bytes())


@pytest.mark.parametrize("k", range(len(UL_STREAMS)))
def test_ul_mode_from_a_spec_dci_format0(k):
    _, recs = run_oracle_ul_stream(k)
    check_ul_records(recs, ul_stream(k)[3])


# ---------------------------------------------------------------------------------------------------------------------------- the transmitter by itself
def test_covering_design_reaches_every_parameter():
    cs = CASES
    built = [case(i) for i in range(NCASES)]
    gs = [(c, s, t) for c, b in zip(cs, built) for s, t in zip(c["grants"], b[3])]
    assert {c["prb"] for c in cs} == {6, 15, 25, 50, 100} and sum(c["prb"] == 100 for c in cs) == 1 and sum(c["prb"] == 50 for c in cs) == 1
    full = [(c, s, t) for c, s, t in gs if c["prb"] == 100]
    assert len(full) == 1 and full[0][1]["L"] == 100 and full[0][2]["seg"]["C"] >= 13
    assert {s["L"] for _, s, _ in gs} == {1, 2, 3, 5, 6, 25, 100}
    assert any(s["n"] == 0 for _, s, _ in gs) and any(s["n"] + s["L"] == c["prb"] and s["L"] < c["prb"] for c, s, _ in gs)
    assert any(12 * s["n"] < 6 * c["prb"] < 12 * (s["n"] + s["L"]) and s["L"] < c["prb"] for c, s, _ in gs)         # carriers on both sides of the centre: k < nre / 2 wraps
    assert {t["Qm"] for _, _, t in gs} == {2, 4, 6, 8}
    assert {t["rv"] for _, _, t in gs} == {0, 1, 2, 3} and {c["cp"] for c in cs} == {0, 1}
    assert {c["cs"] for c in cs} == set(range(8)) and {s["nd"] for _, s, _ in gs} == set(range(8))
    assert any(c["dss"] for c in cs) and len({c["cid"] % 30 for c in cs}) > 5 and len({c["cid"] // 30 for c in cs}) > 5
    assert {c["sf"] for c in cs} == set(range(10))
    assert any(c.get("gh") for c in cs)
    uv = lambda c, s, slot: SU.group_and_sequence(c["cid"], c["dss"], c.get("gh", 0), c.get("sh", 0), 2 * c["sf"] + slot, 12 * s["L"])
    assert any(c.get("gh") and uv(c, s, 0)[0] != uv(c, s, 1)[0] for c, s, _ in gs)                                   # the group does hop between the slots
    assert any(c.get("sh") and s["L"] >= 6 and 1 in (uv(c, s, 0)[1], uv(c, s, 1)[1]) for c, s, _ in gs)              # v = 1 is reached
    assert any(c.get("sh") and s["L"] < 6 and (uv(c, s, 0)[1], uv(c, s, 1)[1]) == (0, 0) for c, s, _ in gs)
    hops = [(c, s, t) for c, s, t in gs if "hop" in s]
    assert {(c["prb"], DCI.hop_bits_format0(c["prb"])) for c, _, _ in hops} == {(25, 1), (50, 2)} and all(c["ho"] for c, _, _ in hops)
    assert all(t["grant"]["n_prb2"] != t["grant"]["n_prb"] for _, _, t in hops)
    u = {(bool(s.get("ack")), bool(s.get("ri")), bool(s.get("cqi"))) for _, s, _ in gs}
    assert {(True, False, False), (False, True, True), (True, True, True)} <= u and {s.get("ack", 0) for _, s, _ in gs} == {0, 1, 2}
    assert all(c["prb"] == 25 and s["cqi"] == 18 for c, s, _ in gs if s.get("cqi")) and _api().o_uci_cqi_bits(25) == 18
    assert any("ia" in s and "ir" in s and "ic" in s for _, s, _ in gs)
    assert any(c["cp"] == 1 and s.get("ack") and s.get("ri") for c, s, _ in gs)
    assert any(s["L"] == 1 and t["q_ack"] == 48 for _, s, t in gs)                                                    # the cap 4 M_sc
    assert any(t["q_cqi"] and t["q_ri"] and t["q_ack"] and np.any(t["punct"]) for _, _, t in gs)
    two = [c for c in cs if len(c["grants"]) > 1]
    assert two and all(a["n"] + a["L"] == b["n"] for c in two for a, b in zip(c["grants"], c["grants"][1:]))         # adjacent PRBs
    assert all(s["mcs"] <= 20 and not s.get("qm") for _, s, _ in gs if s.get("delay")) and {s.get("delay", 0) for _, s, _ in gs} == {0, 1, 2}
    assert all(abs(20 * np.log10(abs(t["gain"]))) <= 3 for _, _, t in gs)
    # every rv decodes alone: the whole mother code fits; and every case leaves the decoder something to work with
    for _, s, t in gs:
        sent = t["G"] - np.count_nonzero(t["punct"])
        assert (t["grant"]["tbs"] + 24) / sent < 0.9
        if t["rv"]:
            assert t["G"] >= 3 * (t["blocks"][0]["K"] + 4)
    assert CASES[NOISY[0]]["grants"][0]["mcs"] == 28 and CASES[NOISY[1]]["grants"][0].get("qm") == 8 and CASES[NOISY[2]]["grants"][0].get("ack")


def test_interleaver_is_a_bijection_on_cells():
    for M, cp, qa, qr, qc in ((12, 0, 48, 0, 0), (36, 1, 32, 25, 91), (72, 0, 13, 13, 48), (60, 0, 28, 22, 80), (24, 0, 0, 96, 190), (12, 1, 48, 48, 72)):
        kind, gidx = SU.interleave(M, cp, qa, qr, qc)
        C_ = SU.n_symb_pusch(cp)
        assert len(kind) == M * C_ and np.sum(kind == SU.RI) == qr and np.sum(kind == SU.ACK) == qa
        written = gidx[kind != SU.RI]
        assert sorted(written) == list(range(M * C_ - qr))                     # every vector g_k lands in exactly one cell
        assert np.all(gidx[kind == SU.CQI] < qc) and np.all(gidx[kind == SU.DATA] >= qc)
        cols = np.arange(M * C_) // M
        assert set(cols[kind == SU.RI]) <= set(SU.COLS_RI[cp]) and set(cols[kind == SU.ACK]) <= set(SU.COLS_ACK[cp])
        rows = np.arange(M * C_) % M
        assert rows[kind == SU.ACK].min() == M - -(-qa // 4) if qa else True   # bottom rows, four cells to a row
    # no control information: transmitted cell (column c, row r) carries vector r C + c
    kind, gidx = SU.interleave(12, 0, 0, 0, 0)
    assert np.array_equal(gidx.reshape(12, 12), np.arange(144).reshape(12, 12).T) and not kind.any()


def test_q_prime_known_answers():
    """the module docstring's hand computations"""
    assert SU.uci_sizes(72, 0, 1056, ri_bits=1, cqi_bits=18) == (0, 13, 48)
    assert SU.uci_sizes(12, 0, 40, nof_ack=1) == (48, 0, 0) and SU.q_prime(1, 12, 12, 20, 40, 10 ** 6) == 72
    assert SU.uci_sizes(36, 1, 232, nof_ack=1, ri_bits=1, cqi_bits=18) == (32, 25, 91)
    assert SU.uci_sizes(60, 0, 2240, nof_ack=2) == (13, 0, 0)
    assert SU.uci_sizes(12, 0, 40, cqi_bits=11)[2] == -(-11 * 144 * 9 // (4 * 40)) and SU.uci_sizes(12, 0, 40, cqi_bits=12)[2] == 144     # L = 8 from O = 12 on; the cap M_sc N_symb
    assert SU.uci_sizes(12, 0, 40, ri_bits=1, cqi_bits=30) == (0, 48, 96)                                                                    # the CQI cap leaves the RI cells out


def test_beta_tables_equal_the_headers():
    hdr = {n: [int(x) for x in _arr("lsn_beta_" + n + "8").split(",")] for n in ("ack", "ri", "cqi")}
    for n, tab in (("ack", SU.BETA_ACK), ("ri", SU.BETA_RI), ("cqi", SU.BETA_CQI)):
        mine = [0 if b is None else b for b in tab] + [0] * (16 - len(tab))
        assert [h / 8 for h in hdr[n]] == mine, n
    assert (SU.BETA_ACK[10], SU.BETA_CQI[8], SU.BETA_RI[11]) == (20, 2.25, 15.875)


def test_dmrs_sequences_have_unit_modulus_and_flat_spectrum():
    for M in (12, 24, 36, 60, 72, 300, 1200):
        for u in (0, 7, 29):
            for v in ((0, 1) if M >= 72 else (0,)):
                r = SU.base_sequence(u, v, M)
                assert np.allclose(np.abs(r), 1.0, atol=1e-12)
                if M >= 36:
                    nzc = max(p for p in range(2, M) if all(p % d for d in range(2, p)))
                    assert np.allclose(np.abs(np.fft.fft(r[:nzc])), np.sqrt(nzc), atol=1e-8), (M, u, v)      # a Zadoff-Chu sequence: constant-amplitude DFT
    assert not np.allclose(SU.base_sequence(3, 0, 72), SU.base_sequence(3, 1, 72))
    # 5.5.1.1 by hand: M_sc = 36, N_ZC = 31, u = 0: qbar = 1, q = 1; u = 1, M_sc = 72, N_ZC = 71: qbar = 142 / 31 = 4.58: q = 5, v = 1: floor(2 qbar) = 9 -> q = 4
    m = np.arange(36) % 31
    assert np.allclose(SU.base_sequence(0, 0, 36), np.exp(-1j * np.pi * m * (m + 1) / 31))
    m = np.arange(72) % 71
    assert np.allclose(SU.base_sequence(1, 1, 72), np.exp(-1j * np.pi * 4 * m * (m + 1) / 71))
    cell = dict(cell_id=100, delta_ss=3, cyclic_shift=5, group_hopping=0, sequence_hopping=0, cp=0)
    assert np.allclose(np.abs(SU.dmrs(cell, 8, 5, 36)), 1.0)


def test_precode_synthesise_demodulate_round_trip():
    rng = np.random.default_rng(4)
    for nprb, cp, n0, L in ((6, 0, 2, 3), (15, 1, 6, 5)):
        M, C_ = 12 * L, SU.n_symb_pusch(cp)
        d = SP.modulate(rng.integers(0, 2, 4 * M * C_), 4)
        z = SU.transform_precode(d, M).reshape(C_, M)
        assert np.allclose(np.sum(np.abs(z) ** 2, axis=1), np.sum(np.abs(d.reshape(C_, M)) ** 2, axis=1))    # 1 / sqrt(M_sc): energy kept
        a = np.zeros((C_ + 2, 12 * nprb), dtype=np.complex128)
        a[:C_, 12 * n0:12 * n0 + M] = z
        back = SU.ideal_demod(SU.scfdma(a, nprb, cp), nprb, cp)
        assert np.allclose(back, a, atol=1e-10)
        zz = back[:C_, 12 * n0:12 * n0 + M]
        i = np.arange(M)
        dd = zz @ np.exp(2j * np.pi * np.outer(i, i) / M) / np.sqrt(M)                                       # the inverse of 5.3.3
        assert np.allclose(dd.reshape(-1), d, atol=1e-9)
    # the half-carrier shift: carrier k(-) = 0 of a 6-PRB cell is the tone at (-36 + 1/2) 15 kHz
    a = np.zeros((14, 72), dtype=np.complex128)
    a[0, 0] = 1
    x = SU.scfdma(a, 6, 0)[10:138]
    assert np.allclose(x * 128, np.exp(2j * np.pi * (-35.5) * np.arange(128) / 128))


def test_format0_known_answers():
    """36.212 5.3.3.1.1.  25 PRB: 9 RIV bits, 23 bits of format 0 against 24 of format 1A, which is an ambiguous size and becomes 25; 6 PRB: 19 against
    20 -> 21; 100 PRB: 27 against 28"""
    assert DCI.size_format0(25) == DCI.size_format1a(25) == 25 and DCI.size_format0(6) == DCI.size_format1a(6) == 21 and DCI.size_format0(100) == 28
    b = DCI.pack_0(25, 3, 2, 17, ndi=1, tpc=2, cyclic_shift=5, cqi_request=1)
    assert b == [0, 0] + [0, 0, 0, 0, 1, 1, 1, 0, 0] + [1, 0, 0, 0, 1] + [1] + [1, 0] + [1, 0, 1] + [1] + [0, 0]              # RIV = 25 + 3 = 28
    b = DCI.pack_0(25, 3, 2, 17, hop=0)
    assert b[:2] == [0, 1] and b[2] == 0 and b[3:11] == [0, 0, 0, 1, 1, 1, 0, 0]                                       # one hopping bit, eight RIV bits
    b = DCI.pack_0(50, 20, 6, 9, hop=1)
    assert DCI.riv_bits(50) == 11 and b[2:4] == [0, 1] and b[4:13] == [int(x) for x in format(50 * 5 + 20, "09b")]
    assert [DCI.hop_bits_format0(n) for n in (6, 49, 50, 100)] == [1, 1, 2, 2]


def test_dci_format0_size_equals_the_oracles():
    from lsn_testlib import oracle
    for nprb in (6, 15, 25, 50, 75, 100):
        cell = OCell(nprb, 1, 1, 1, 0, 0)
        assert DCI.size_format0(nprb) == oracle().o_dci_format_sizeof(C.byref(cell), 0)


# Type-1 hopping, documented reference behaviour.  36.213 8.4.1 defines the slot-0 position as RB_START = ntilde^S1 + Ntilde_HO / 2, applies
# Table 8.4-2 to ntilde^S1 modulo N_RB^PUSCH and adds Ntilde_HO / 2 back.  The reference (ul_sniffer_pusch.c:58, "n_prb_1_tilde = n_prb_1") applies the table to
# RB_START itself and adds nothing back; oracle, product and pusch_hop_slot1 follow the reference.  The two agree whenever the sum does not wrap differently,
# i.e. with pusch-HoppingOffset 0 always, and with an offset for every RB_START except the Ntilde_HO / 2 positions below a wrap.  HOP_DEPARTS lists, for the two
# cells of the hopping cases, exactly the RB_START values where they differ.
HOP_DEPARTS = {(25, 2, 0): [11], (50, 4, 0): [35, 36], (50, 4, 1): [11, 12], (50, 4, 2): [23, 24]}


def test_type1_hopping_offset_against_the_letter_of_the_specification():
    for (nprb, ho, bits), want in HOP_DEPARTS.items():
        ht = ho + ho % 2
        starts = range(ht // 2, nprb - nprb % 2 - ht // 2)
        assert [s for s in starts if SU.hop_slot1_spec(nprb, ho, bits, s) != pusch_hop_slot1(nprb, ho, bits, s)] == want, (nprb, ho, bits)
    for nprb in (25, 50, 100):      # no offset: no difference
        for bits in range(DCI.hop_bits_format0(nprb) * 2 - 1):
            assert all(SU.hop_slot1_spec(nprb, 0, bits, s) == pusch_hop_slot1(nprb, 0, bits, s) for s in range(nprb - nprb % 2))
    for c in CASES:                 # the hopping cases sit where both readings agree
        for s in c["grants"]:
            if "hop" in s:
                assert SU.hop_slot1_spec(c["prb"], c["ho"], s["hop"], s["n"]) == pusch_hop_slot1(c["prb"], c["ho"], s["hop"], s["n"])

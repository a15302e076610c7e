"""The oracle's PDSCH chain (DCI unpacking, grant conversion, demodulator, rate de-matching, turbo decoder) against an independent transmitter written
from the specifications (tests/spec_pdsch.py, tests/spec_dci.py, rendered by tests/spec_downlink.py).

Every other test of the downlink data path loops the oracle back on tools/txgen, which shares its reading of TS 36.211 / 36.212 / 36.213 with the oracle
and the product.  Here the truth is what the spec transmitter sent, and every check is exact (in the band-edge zone: an exact count, EDGE_BAD): the MAC-LTE records are the transmitted transport
blocks, every descrambled soft bit has the sign of the transmitted rate-matched bit and is not zero, K / F / E / rv of every code block equal the
independent segmentation, the de-rate-matched streams have the encoder's signs where the redundancy version covers a position and are exactly 0
where it does not, and every block CRC passes.  tests/test_gpu_spec_pdsch.py puts the same streams through the HIP kernels.

No transport block size a DCI can signal needs filler bits or two block sizes K+ / K- (tests/test_spec_tables.py: the table was built from the
interleaver sizes; test_no_table_size_needs_fillers_or_two_block_sizes), so the filler / <NULL> placement and the K+ / K- split are checked on the
oracle's block-level entry points instead (test_filler_bits_at_block_level, test_segmentation_equals_the_oracles).

Three documented departures of the receiver, each reference behaviour, are asserted where they occur and nowhere else: the
band-edge zone of the channel estimate (EDGE, EDGE_BAD), a grant whose first transport block is disabled (NOT_DECODED), P_B on one port (ONE_PORT_POWER).

AWGN cases (a condition on the inputs, not a tolerance): NOISY_SNR_DB = 26 dB (noise variance 10^-2.6 per resource element against unit CRS
energy) on cases NOISY.  Swept on the CPU in 1 dB steps from 30 dB down with the seeds of the cases: the first payload is lost at 18 dB (case 4: 64QAM at
rate 0.85, three blocks), 20 dB (case 7: the 16QAM codeword of a CDD pair) and 18 dB (case 17: 256QAM at rate 0.77); every step above decodes.  26 dB
is 6 dB above the first failure of the weakest case."""
import ctypes as C
import functools

import numpy as np
import pytest

import spec_dci as DCI
import spec_downlink as SD
import spec_pdsch as SP
from lsn_testlib import OCbSegm, OCell, OGrant, OracleWorker, oracle, oracle_trace, oracle_trace_enable, parse_pcap
from test_spec_control_oracle import _rnti_for

NOISY = (4, 7, 17)
NOISY_SNR_DB = 26.0
FMT_IDX = {"1": 1, "1A": 2, "2": 6, "2A": 7}     # the oracle's format numbers (oracle/lsn_oracle.h)
ALL = "all"

# One subframe per case.  fmt: the DCI format ("SI": format 1A with SI-RNTI); alloc: (first PRB, length) for type 2, a set of RBGs (or ALL) for type 0;
# tb: (MCS, rv) per transport block, None = disabled; t256: the UE uses the 256QAM table; pmi: the codebook index (36.211 Table 6.3.4.2.3-1)
CASES = [
    dict(prb=6, ports=1, cp=0, rx=1, cfi=3, cid=300, sf=0, fmt="1A", alloc=(0, 6), tb=[(2, 0)]),                      # 0: four control symbols, subframe 0, the whole (= centre) band
    dict(prb=6, ports=2, cp=1, rx=2, cfi=2, cid=301, sf=5, fmt="1", alloc=ALL, tb=[(12, 0)]),                         # 1: subframe 5, extended CP, RBG size 1
    dict(prb=15, ports=2, cp=0, rx=1, cfi=2, cid=152, sf=0, fmt="1A", alloc=(4, 7), tb=[(19, 0)]),                    # 2: odd bandwidth, the PRBs the centre 72 subcarriers touch
    dict(prb=25, ports=4, cp=0, rx=2, cfi=2, cid=447, sf=5, fmt="1", alloc={4, 5, 6, 7}, tb=[(10, 0)]),               # 3: SFBC-FSTD over the PSS / SSS
    dict(prb=25, ports=2, cp=0, rx=1, cfi=1, cid=100, sf=3, fmt="1", alloc=ALL, tb=[(28, 0)]),                        # 4: three code blocks, full band, short last RBG
    dict(prb=25, ports=2, cp=1, rx=1, cfi=3, cid=503, sf=7, fmt="1A", alloc=(7, 1), tb=[(0, 0)]),                     # 5: one PRB, K = 40, E > K_w
    dict(prb=15, ports=1, cp=1, rx=2, cfi=2, cid=11, sf=2, fmt="1", alloc=ALL, tb=[(0, 0)]),                          # 6: a small block on the full band: repetition
    dict(prb=15, ports=2, cp=0, rx=2, cfi=2, cid=34, sf=4, fmt="2A", alloc={1, 2, 5}, tb=[(14, 0), (8, 0)]),          # 7: large-delay CDD, 16QAM + QPSK
    dict(prb=25, ports=2, cp=1, rx=2, cfi=1, cid=262, sf=9, fmt="2A", alloc={0, 3, 12}, tb=[(18, 0), (5, 0)], swap=1),  # 8: CDD, swapped, 64QAM + QPSK
    dict(prb=15, ports=2, cp=0, rx=1, cfi=3, cid=5, sf=1, fmt="2A", alloc={2, 3}, tb=[(11, 0), None]),                # 9: format 2A, one block -> transmit diversity
    dict(prb=25, ports=4, cp=0, rx=1, cfi=1, cid=419, sf=6, fmt="2A", alloc={1, 9}, tb=[None, (7, 0)], gated=1),      # 10: four ports, block 2 alone: never decoded (NOT_DECODED)
    dict(prb=6, ports=2, cp=0, rx=1, cfi=2, cid=88, sf=8, fmt="2", alloc={0, 1, 2}, tb=[(6, 0), None], pmi=0),         # 11-14: closed loop, one layer, codebook index 0..3
    dict(prb=15, ports=2, cp=1, rx=2, cfi=2, cid=196, sf=3, fmt="2", alloc={0, 7}, tb=[(13, 0), None], pmi=1),
    dict(prb=15, ports=2, cp=0, rx=1, cfi=2, cid=77, sf=6, fmt="2", alloc={3, 4}, tb=[(19, 0), None], pmi=2),
    dict(prb=25, ports=2, cp=0, rx=2, cfi=3, cid=150, sf=2, fmt="2", alloc={5, 6}, tb=[(9, 0), None], pmi=3),
    dict(prb=15, ports=2, cp=0, rx=2, cfi=3, cid=301, sf=7, fmt="2", alloc={0, 1, 6}, tb=[(15, 0), (4, 0)], pmi=1),    # 15, 16: closed loop, two layers, codebook index 1, 2
    dict(prb=25, ports=2, cp=1, rx=2, cfi=2, cid=5, sf=4, fmt="2", alloc={2, 11}, tb=[(7, 0), (21, 0)], pmi=2, swap=1),
    dict(prb=15, ports=2, cp=0, rx=2, cfi=2, cid=503, sf=8, fmt="1", alloc={1, 2}, tb=[(22, 0)], t256=True),          # 17: 256QAM, found by the second table attempt
    dict(prb=6, ports=2, cp=0, rx=1, cfi=3, cid=34, sf=1, fmt="2", alloc={4, 5}, tb=[(3, 0), None], pmi=None),        # 18: format 2, one block, precoding information 0 -> transmit diversity
    dict(prb=50, ports=2, cp=0, rx=1, cfi=2, cid=262, sf=9, fmt="1", alloc={0, 8, 16}, tb=[(9, 0)]),                  # 19: RBG size 3, the short last RBG
    dict(prb=100, ports=4, cp=0, rx=2, cfi=1, cid=11, sf=2, fmt="1", alloc={3, 24}, tb=[(15, 0)]),                    # 20: RBG size 4
    dict(prb=25, ports=1, cp=0, rx=1, cfi=2, cid=196, sf=4, fmt="1", alloc={0, 6, 12}, tb=[(17, 0)]),                 # 21: one port, 64QAM
    dict(prb=6, ports=1, cp=0, rx=1, cfi=2, cid=150, sf=5, fmt="SI", alloc=(1, 4), tb=[(3, 0)], n1a=3),               # 22-25: SI-RNTI, rv 0, 2, 3, 1, each decoded alone
    dict(prb=15, ports=2, cp=1, rx=2, cfi=3, cid=419, sf=5, fmt="SI", alloc=(9, 5), tb=[(4, 2)], n1a=2),
    dict(prb=25, ports=4, cp=0, rx=1, cfi=3, cid=88, sf=0, fmt="SI", alloc=(2, 6), tb=[(3, 3)], n1a=3),
    dict(prb=15, ports=1, cp=0, rx=1, cfi=2, cid=77, sf=1, fmt="SI", alloc=(0, 4), tb=[(2, 1)], n1a=2),
    dict(prb=25, ports=1, cp=0, rx=1, cfi=2, cid=196, sf=4, fmt="1", alloc={3, 6, 9}, tb=[(21, 0)], t256=True, pb=1),  # 26: one port, 256QAM (ONE_PORT_POWER)
]
NCASES = len(CASES)
# ONE_PORT_POWER, documented reference behaviour: before an RRC set-up is seen the receiver takes P_B = 1 on every cell (SubframeWorker.cc:372),
# which on ONE port means rho_B / rho_A = 4/5 (36.213 Table 5.2-1); the transmitter here sends P_B = 0 (rho_B = rho_A).  The receiver therefore scales the
# symbols that carry CRS up by sqrt(5/4): QPSK, 16QAM and 64QAM keep every decision (the outermost 64QAM level 7 -> 7.83 stays above 6), 256QAM does not
# (11 -> 12.3 crosses 12: b4 / b5 turn; 13 -> 14.5 crosses 14: b6 / b7 turn; 9 -> 10.06 sits on the threshold 10: the last bit is 0 or +-1).  The case marked
# pb=1 asserts exactly those bits turned on those symbols, the on-threshold bits within +-1, and every other soft bit right (expected_bits).
# NOT_DECODED, documented reference behaviour: PDSCH_Decoder::decode_dl_mode only decodes a grant whose FIRST transport block has a size
# (DL_Sniffer_PDSCH.cc:887), so a format 2 / 2A grant that disables block 1 and sends block 2 (36.212 5.3.3.1.5: I_MCS = 0, rv = 1) is accepted as a DCI
# and then dropped: no decode call, no record.  Cases marked gated=1 assert exactly that.


def _scheme(c):
    """-> (scheme, codewords as indices into tb, pmi) from 36.213 7.1 (transmission modes 1-4) for the DCI format and the enabled blocks"""
    en = [i for i, t in enumerate(c["tb"]) if t is not None]
    if c["fmt"] in ("1", "1A", "SI"):
        return ("port0" if c["ports"] == 1 else "txd"), en, 0
    if len(en) == 1:
        if c["fmt"] == "2A" or c.get("pmi") is None:
            return "txd", en, 0
        return "mux1", en, c["pmi"]
    cw = en[::-1] if c.get("swap") else en      # 36.212 Table 5.3.3.1.5-1: swap flag 1 puts transport block 1 on codeword 1, block 2 on codeword 0
    return ("cdd", cw, 0) if c["fmt"] == "2A" else ("mux2", cw, c["pmi"])


@functools.lru_cache(maxsize=None)
def case(i, snr_db=None):
    """-> (p: the cell and subframe, iq, truth of control_subframe + pdsch channel, records [(rnti, tti, bytes)], the DCI (L, ncce, rnti, bits))"""
    c = CASES[i]
    rng = np.random.default_rng(7000 + i)
    p = dict(nof_prb=c["prb"], nof_ports=c["ports"], cp=c["cp"], nof_rx=c["rx"], cfi=c["cfi"], cell_id=c["cid"], sf_idx=c["sf"], sfn=300 + 7 * i, ng_x6=1)
    reg = SD.ControlRegion(c["prb"], c["ports"], c["cid"], c["cp"], 1)
    ncce = reg.nof_cce(c["cfi"])
    nctrl = reg.nof_symbols(c["cfi"])
    scheme, cws, pmi = _scheme(c)
    # the DCI: SI-RNTI at level 4 on CCE 0 (common space); a new C-RNTI at level 8 (4 on a small cell) on a location that is valid for it, so that FALCON's
    # shortcut rule activates it at first sight
    if c["fmt"] == "SI":
        L, n, rnti = 4, 0, SD.SI_RNTI
    else:
        assert ncce >= 4, ("SET-UP: no level-4 location", i, ncce)
        found = next(((L, n, r) for L in (8, 4) for n in range(0, min(ncce, 84) - L + 1, L) for r in [_rnti_for(ncce, L, n, c["sf"], rng)] if r is not None), None)
        if found:
            L, n, rnti = found
        else:    # a dozen CCEs or fewer: the six level-2 candidates of any RNTI cover every level-4 location ("ambiguous"; accepted all the same)
            L, n = 4, 0
            rnti = next(r for r in (int(v) for v in rng.integers(0x000B, 0xFFF4, 4000)) if SD.validate_location(ncce, 0, L, c["sf"], r) == 1)
            assert ncce // 2 <= 6
    # transport blocks: sizes from 36.213 7.1.7 (SI-RNTI: the MCS field is I_TBS, the column N_PRB^1A, QPSK)
    P = DCI.rbg_size(c["prb"])
    nrbg = -(-c["prb"] // P)
    rbgs = set(range(nrbg)) if c["alloc"] == ALL else c["alloc"]
    if c["fmt"] == "SI":
        bits, prbs = DCI.pack_1a_si(c["prb"], c["alloc"][0], c["alloc"][1], c["tb"][0][0], c["tb"][0][1], c["n1a"])
        sizes = [(2, SP.tbs_of(c["tb"][0][0], c["n1a"])[1])]
    else:
        if c["fmt"] == "1A":
            bits, prbs = DCI.pack_1a(c["prb"], c["alloc"][0], c["alloc"][1], *c["tb"][0], harq=i % 8, ndi=i % 2)
        elif c["fmt"] == "1":
            bits, prbs = DCI.pack_1(c["prb"], rbgs, *c["tb"][0], harq=i % 8, ndi=i % 2, tpc=i % 4)
        else:
            tbf = [(t[0], t[1], (i + k) % 2) if t else (0, 1, 0) for k, t in enumerate(c["tb"])]
            pinfo = 0 if c["ports"] == 4 or c["fmt"] == "2A" else DCI.precoding_info_2ports(len(cws), scheme, pmi)
            bits, prbs = DCI.pack_2x(c["fmt"], c["prb"], c["ports"], rbgs, tbf[0], tbf[1], swap=c.get("swap", 0), pinfo=pinfo, harq=i % 8, tpc=i % 4)
        sizes = [SP.tbs_of(t[0], len(prbs), c.get("t256", False)) if t else None for t in c["tb"]]
    payload = [rng.integers(0, 2, s[1]).astype(np.uint8) if s else None for s in sizes]
    ch = SP.build(c["prb"], c["ports"], c["cid"], c["cp"], c["sf"], nctrl, rnti, prbs, scheme,
                  [dict(bits=payload[t], Qm=sizes[t][0], rv=c["tb"][t][1]) for t in cws], pmi)
    ch["tb_of_cw"] = cws
    iq, truth = SD.control_subframe(dcis=[(L, n, rnti, np.array(bits, dtype=np.uint8))], seed=i, snr_db=snr_db, pdsch=[ch],
                                    **{k: v for k, v in p.items()})
    tti = 10 * p["sfn"] + p["sf_idx"]
    records = [] if c.get("gated") else [(rnti, tti, np.packbits(b).tobytes()) for b in payload if b is not None]
    return p, iq, truth, records, (L, n, rnti, bits)


def ocell(p):
    return OCell(p["nof_prb"], p["nof_ports"], p["cell_id"], p["ng_x6"], 0, p["cp"])


# ---------------------------------------------------------------------------------------------------------------------------- checks shared with the GPU file
def check_accepted(acc, i, dci):
    """the DCI of the case is among the accepted ones: a search miss must read as a set-up error, not as a PDSCH failure"""
    L, n, rnti, bits = dci
    fmt = FMT_IDX["1A" if CASES[i]["fmt"] == "SI" else CASES[i]["fmt"]]
    hit = [a for a in acc if (int(a[0]), int(a[1]), int(a[3]), int(a[4])) == (rnti, fmt, n, len(bits))]
    assert len(hit) == 1, ("SET-UP: the DCI was not accepted", i, hex(rnti), [tuple(int(v) for v in a) for a in acc if a[0]])


def matching_jobs(jobs, ch, tti):
    """the decode calls made with what was transmitted: RNTI, TTI, the resource elements and the modulation of each codeword"""
    qm = [cw["Qm"] for cw in ch["cw"]] + [0] * (2 - len(ch["cw"]))
    return [j for j in jobs if (j["tti"], j["rnti"], j["nof_re"], list(j["qm"])) == (tti, ch["rnti"], len(ch["res"]), qm) and j.get("have", True)]


# Band-edge channel estimate, documented reference behaviour.  The channel estimator smooths the pilots of a port with five taps over
# a zero-padded row, as the reference's srsRAN does.  On a flat channel the outermost pilot of either side comes out 30 % low and the next one 5 % low; the third
# is exact.  Pilots sit six subcarriers apart at an offset of 0..5, so every estimate that interpolates or extrapolates an outermost pilot lies in
# k <= 10 or k >= 12 N_RB - 11: the zone.  (The 5 % of the second pilot is less than half a level step even for the outermost 256QAM level, 0.05 x 15 < 1.)
# A real, positive gain error cannot turn a sign bit b0 / b1 under single-port reception, whatever the modulation; under transmit diversity the gain errors
# a, b of the two ports leak the partner symbol in with weight |b - a| |h0| |h1| <= 0.31 |h0| |h1| against a |h0|^2 + b |h1|^2 >= 1.38 |h0| |h1|, which QPSK survives
# and an inner level of a larger constellation need not.  So: outside the zone every soft bit is judged; inside it every soft bit is judged as well, the sign
# bits of single-port codewords and every bit of QPSK under single-port / transmit-diversity reception must be right, and the number of zero and of
# wrong-signed soft bits of each remaining codeword is the number written down here (oracle and kernels are bit-identical, so it holds for both).
EDGE = 11
EDGE_BAD = {(1, 0): (1, 0), (4, 0): (8, 139), (8, 1): (7, 102), (12, 0): (11, 7), (15, 0): (0, 3), (21, 0): (5, 125)}   # (case, codeword): (zero, wrong); else (0, 0)


def pb_symbols(i):
    """the symbols with CRS of port 0 (36.211 6.10.1.2: symbols 0 and N_symb - 3 of each slot) of a case marked pb=1, else ()"""
    nsl = 6 if CASES[i]["cp"] else 7
    return (0, nsl - 3, nsl, 2 * nsl - 3) if CASES[i].get("pb") else ()


def expected_bits(ch, cw, symbols):
    """ONE_PORT_POWER: the descrambled bits an ideal demapper returns when the elements of `symbols` arrive sqrt(5/4) too large: each of I, Q goes to the
    nearest constellation level (the outermost beyond it), e.g. at 256QAM 11 -> 12.3 reads as 13 (b4 / b5 turn) and 13 -> 14.5 as 15 (b6 / b7 turn); every other
    level, and every level of the smaller constellations, reads as itself - except 9, which lands on 10.06, six hundredths of a level past the threshold 10:
    its last bit (b6 for I, b7 for Q) is on the threshold, a soft bit of 0 or +-1 (0.06 x 0.0767 x 180 = 0.86 before rounding).
    -> (bits[G], on_threshold[G])"""
    Qm = cw["Qm"]
    if not symbols:
        return cw["f"], np.zeros(cw["G"], dtype=bool)
    n, top = 1 << Qm, (1 << (Qm // 2)) - 1
    pat = np.array([[(v >> (Qm - 1 - k)) & 1 for k in range(Qm)] for v in range(n)], dtype=np.uint8)
    norm = np.sqrt(2.0 * np.mean(np.arange(1, top + 1, 2) ** 2.0))
    pts = np.rint(SP.modulate(pat.reshape(-1), Qm) * norm)
    lut = np.zeros((top + 1, top + 1), dtype=np.int64)
    lut[((pts.real + top) // 2).astype(int), ((pts.imag + top) // 2).astype(int)] = np.arange(n)
    on = np.array([l in symbols for l, _ in ch["res"]])
    x0 = SP.modulate(cw["f"] ^ cw["c"], Qm) * norm
    x = x0 * np.where(on, np.sqrt(1.25), 1.0)
    level = lambda v: np.sign(v) * (2 * np.minimum(np.floor(np.abs(v) / 2), top // 2) + 1)
    idx = lut[((level(x.real) + top) // 2).astype(int), ((level(x.imag) + top) // 2).astype(int)]
    hair = np.zeros((len(x), Qm), dtype=bool)
    if Qm == 8:
        hair[:, 6], hair[:, 7] = on & (np.rint(np.abs(x0.real)) == 9), on & (np.rint(np.abs(x0.imag)) == 9)
    return pat[idx].reshape(-1) ^ cw["c"], hair.reshape(-1)


def check_job(job, ch, nre, i):
    """checks (b) and (c) on one decode call of case i -> (code blocks checked, soft bits judged)"""
    nchk = njudged = 0
    k = np.array([kk for _, kk in ch["res"]])
    for q, cw in enumerate(ch["cw"]):
        Qm = cw["Qm"]
        llr = job["llr"][q].astype(np.int64)
        assert len(llr) == cw["G"], (len(llr), cw["G"])
        want, hair = expected_bits(ch, cw, pb_symbols(i))
        if pb_symbols(i):
            assert hair.any() and np.all(np.abs(llr[hair]) <= 1), ("ONE_PORT_POWER: level 9 on the threshold", int(np.abs(llr[hair]).max()))
            turned = np.nonzero((want != cw["f"]) & ~hair)[0]
            assert turned.size and set(turned % Qm) == {4, 5, 6, 7} and {ch["res"][x // Qm][0] for x in turned} <= set(pb_symbols(i))
        zone = np.repeat((k < EDGE) | (k >= nre - EDGE), Qm)
        bit = np.arange(cw["G"]) % Qm
        where = lambda m: [(ch["res"][x // Qm], int(x % Qm), int(llr[x])) for x in np.nonzero(m)[0][:8]]
        # (b) the oracle's header: positive = bit 1 (o_pdsch.c, demod_llr)
        zero, wrong = (llr == 0) & ~hair, (llr != 0) & ((llr > 0) != (want == 1)) & ~hair
        assert not np.any(zero & ~zone), ("zero soft bits", q, int(np.sum(zero & ~zone)), where(zero & ~zone))
        assert not np.any(wrong & ~zone), ("soft-bit signs", q, int(np.sum(wrong & ~zone)), where(wrong & ~zone))
        sure = np.ones(cw["G"], dtype=bool) if Qm == 2 and ch["scheme"] in ("port0", "txd") else (bit < 2) if ch["scheme"] == "port0" else np.zeros(cw["G"], dtype=bool)
        assert not np.any((zero | wrong) & sure), ("soft bits the band edge cannot turn", q, where((zero | wrong) & sure))
        got = (int(np.sum(zero & zone)), int(np.sum(wrong & zone)))
        assert got == EDGE_BAD.get((i, q), (0, 0)), ("zero / wrong soft bits in the band-edge zone", i, q, got, EDGE_BAD.get((i, q), (0, 0)), where((zero | wrong) & zone))
        njudged += cw["G"]
        # (c): a position of d3 that a zero, wrong or (ONE_PORT_POWER) turned soft bit feeds is not judged for its sign
        off = zero | wrong | (want != cw["f"]) | hair
        cbs = [cb for cb in job["cbs"] if cb["tb"] == ch["tb_of_cw"][q]]
        assert len(cbs) == cw["seg"]["C"], (len(cbs), cw["seg"]["C"])
        o = 0
        for r, (cb, t) in enumerate(zip(cbs, cw["blocks"])):
            assert (cb["K"], cb["F"], cb["E"], cb["rv"]) == (t["K"], t["F"], t["E"], cw["rv"]), (q, r, cb["K"], cb["F"], cb["E"], cb["rv"], t["K"], t["F"], t["E"])
            check_d3(cb["d3"], t, off[o:o + t["E"]])
            o += t["E"]
            assert cb["ok"] == 1, ("block CRC", q, r)
            nchk += 1
    return nchk, njudged


def check_d3(d3, t, exempt=None):
    """the de-rate-matched streams of one block against the encoder's d(0..2): signs where the redundancy version covers a position (tail included),
    exactly 0 where it does not, the known-zero value -511 on filler positions.  exempt[E]: the soft bits check_job found zero or wrong (their number is
    asserted there); a position one of them feeds is not judged for its sign"""
    d = t["d"].reshape(-1)
    got = np.asarray(d3, dtype=np.int64).reshape(-1)
    assert got.shape == d.shape
    cov = np.zeros(d.size, dtype=bool)
    cov[t["src"]] = True
    fill = d == SP.NULL
    assert not cov[fill].any()
    judged = cov.copy()
    if exempt is not None:
        judged[t["src"][exempt]] = False
    assert np.array_equal(got[judged] > 0, d[judged] == 1) and not np.any(got[judged] == 0), ("d3 signs", int(np.sum((got[judged] > 0) != (d[judged] == 1))))
    assert not np.any(got[~cov & ~fill]), ("d3 not 0 where the redundancy version sends nothing", int(np.count_nonzero(got[~cov & ~fill])))
    assert np.all(got[fill] == -511)


def check_records(recs, want):
    """(a) the records are exactly the transmitted transport blocks"""
    got = [(r["rnti"], 10 * r["sfn"] + r["sf"], r["pdu"]) for r in recs]
    assert len(got) == len(want), ("records", [(hex(a), b, len(c)) for a, b, c in got], [(hex(a), b, len(c)) for a, b, c in want])
    for g, w in zip(got, want):
        assert g[:2] == w[:2] and g[2] == w[2], ("record", hex(g[0]), g[1], len(g[2]), hex(w[0]), w[1], len(w[2]))


def run_oracle_case(p, iq):
    oracle_trace_enable(True)
    ow = OracleWorker(p["nof_prb"], p["nof_ports"], p["cell_id"], p["nof_rx"], p["ng_x6"], cp=p["cp"])
    ow.work(iq, 10 * p["sfn"] + p["sf_idx"])
    tr = oracle_trace()
    oracle_trace_enable(False)
    return ow, tr


# ---------------------------------------------------------------------------------------------------------------------------- the transmitter by itself
def test_crc_of_message_plus_parity_is_zero():
    rng = np.random.default_rng(1)
    for poly in (SP.G_CRC24A, SP.G_CRC24B):
        for n in (1, 16, 40, 333, 6120):
            m = list(rng.integers(0, 2, n))
            assert SP.crc24(m + SP.crc24(m, poly), poly) == [0] * 24
        assert SP.crc24([1], poly) == [int(b) for b in format(poly & 0xFFFFFF, "024b")]   # a one-bit message leaves the polynomial


def test_subblock_interleaver_and_selection_are_a_bijection():
    """E = K_w - N_null at rv 0 reads every non-NULL position of the circular buffer exactly once"""
    rng = np.random.default_rng(2)
    for K, F in ((40, 0), (48, 5), (512, 0), (1056, 17), (6144, 0), (2112, 40)):
        c = rng.integers(0, 2, K).astype(np.uint8)
        c[:F] = SP.NULL
        d = SP.turbo_encode(c)
        w, R = SP.circular_buffer(K + 4)
        assert sorted(w[w >= 0]) == list(range(3 * (K + 4))) and len(w) == 96 * R
        n = 3 * (K + 4) - 2 * F
        e, src = SP.rate_match(d, n, 0)
        assert sorted(src) == sorted(np.nonzero(d.reshape(-1) != SP.NULL)[0]) and not np.any(e == SP.NULL)


def test_turbo_encoder_known_answers():
    """hand-checkable points: a single 1 at position 0 gives the impulse response of g1 / g0 = (1 + D + D^3) / (1 + D^2 + D^3), period 7; the twelve tail bits
    drive both registers back to zero, so an all-zero block has an all-zero tail"""
    d = SP.turbo_encode(np.array([1] + [0] * 39, dtype=np.uint8))
    assert d[1, :15].tolist() == [1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0] and d[0, :40].tolist() == [1] + [0] * 39
    assert not SP.turbo_encode(np.zeros(40, dtype=np.uint8)).any()
    assert SP.qpp(40)[:4].tolist() == [0, 13, 6, 19] and sorted(SP.qpp(6144)) == list(range(6144))   # Table 5.1.3-3, K = 40: f1 = 3, f2 = 10


def test_segmentation_known_answers():
    assert SP.segment(16) == dict(C=1, Kp=40, Km=0, Cp=1, Cm=0, F=0, L=0, Ks=[40])
    s = SP.segment(18336)      # 25 PRB, MCS 28: B = 18360 -> C = 3, B' = 18432 = 3 x 6144
    assert (s["C"], s["F"]) == (3, 0) and sum(s["Ks"]) == 18336 + 24 + 72
    s = SP.segment(6200)       # B = 6224 -> two blocks, B' = 6272 = 3136 x 2
    assert (s["C"], s["Kp"], s["Km"], s["F"]) == (2, 3136, 3072, 0)
    s = SP.segment(6121)       # not a table size: B = 6145 -> B' = 6193, K+ = 3136, K- = 3072: C- = 1, F = 15
    assert (s["C"], s["Cm"], s["Cp"], s["F"]) == (2, 1, 1, 3136 + 3072 - 6193)


def test_no_table_size_needs_fillers_or_two_block_sizes():
    for row in SP._TBS_FILE:
        for tbs in set(row):
            s = SP.segment(tbs)
            assert s["F"] == 0 and s["Cm"] == 0, (tbs, s)


def test_segmentation_equals_the_oracles():
    """36.212 5.1.2 on sizes no grant carries: fillers, and K- blocks in front of K+ blocks"""
    seen = set()
    for tbs in list(range(16, 6200, 8)) + list(range(6100, 100000, 104)) + [6121, 12200, 12345]:
        o, s = OCbSegm(), SP.segment(tbs)
        assert oracle().o_cbsegm(C.byref(o), tbs) == 0
        assert (o.C, o.Cp, o.Cm, o.Kp, o.F) == (s["C"], s["Cp"], s["Cm"], s["Kp"], s["F"]) and (o.Km == s["Km"] or o.Cm == 0), (tbs, s)
        seen |= {("F", s["F"] > 0), ("two", s["Cm"] > 0 and s["Cp"] > 0)}
    assert {("F", True), ("two", True)} <= seen


def test_constellations_have_unit_power_and_gray_neighbours():
    for Qm in (2, 4, 6, 8):
        n = 1 << Qm
        b = np.array([[(v >> (Qm - 1 - k)) & 1 for k in range(Qm)] for v in range(n)], dtype=np.uint8)
        x = SP.modulate(b.reshape(-1), Qm)
        assert abs(np.mean(np.abs(x) ** 2) - 1.0) < 1e-12 and len(set(np.round(x, 9))) == n
        step = 2.0 / np.sqrt(2.0 * np.mean(np.arange(1, 2 ** (Qm // 2), 2) ** 2.0))
        for a in range(n):
            near = np.nonzero(np.abs(np.abs(x - x[a]) - step) < 1e-9)[0]
            assert len(near) >= 2 and all(int(np.sum(b[a] != b[o])) == 1 for o in near), (Qm, a)
    # 36.211 Table 7.1.2-1 .. 7.1.4-1, first rows and one inner row each
    assert np.allclose(SP.modulate([0, 0, 0, 1, 1, 0, 1, 1], 2) * np.sqrt(2), [1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j])
    assert np.allclose(SP.modulate([0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1], 4) * np.sqrt(10), [1 + 1j, 3 + 1j, -1 - 3j])
    assert np.allclose(SP.modulate([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0], 6) * np.sqrt(42), [3 + 3j, 3 + 5j, 7 + 3j])
    assert np.allclose(SP.modulate([0] * 8 + [0, 0, 0, 0, 0, 0, 1, 0] + [1, 0, 1, 0, 1, 0, 1, 0], 8) * np.sqrt(170), [5 + 5j, 7 + 5j, -15 + 5j])


def test_dci_sizes_equal_the_oracles():
    for nprb in SD.BANDWIDTHS:
        for ports in (1, 2, 4):
            cell = OCell(nprb, ports, 1, 1, 0, 0)
            fmts = [("0", 0), ("1A", 2), ("1", 1)] + ([("2", 6), ("2A", 7)] if ports > 1 else [])
            for f, idx in fmts:
                assert DCI.sizeof(f, nprb, ports) == oracle().o_dci_format_sizeof(C.byref(cell), idx), (nprb, ports, f)


def test_riv_and_bitmap_known_answers():
    assert DCI.riv(25, 0, 1) == 0 and DCI.riv(25, 3, 2) == 28 and DCI.riv(25, 0, 25) == 25 * 1 + 24 and DCI.riv(6, 1, 5) == 6 * 2 + 4
    assert [DCI.rbg_size(n) for n in (6, 10, 11, 26, 27, 63, 64, 110)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert DCI.type0_field(25, {0, 12}) == ([0, 1] + [0] * 11 + [1], [0, 1, 24]) and DCI.type0_field(6, {5})[0] == [0, 0, 0, 0, 0, 1]
    assert DCI.type0_field(50, {16})[1] == [48, 49]


def test_covering_design_reaches_every_parameter():
    cs = CASES
    built = [case(i) for i in range(NCASES)]
    chans = [b[2]["pdsch"][0] for b in built]
    assert sum(bool(c.get("pb")) for c in cs) == 1
    assert {c["ports"] for c in cs} == {1, 2, 4} and {c["rx"] for c in cs} == {1, 2} and {c["cp"] for c in cs} == {0, 1}
    assert {c["cfi"] for c in cs} == {1, 2, 3} and any(c["prb"] == 6 and c["cfi"] == 3 for c in cs)                  # four control symbols
    assert {c["cid"] % 6 for c in cs} == set(range(6))
    centre = lambda c, ch: set(ch["prbs"]) >= set(range((6 * c["prb"] - 36) // 12, (6 * c["prb"] + 35) // 12 + 1))   # every PRB the centre 72 subcarriers touch
    for sf in (0, 5):
        assert any(c["sf"] == sf and c["prb"] == 6 and centre(c, ch) for c, ch in zip(cs, chans))
        assert any(c["sf"] == sf and c["prb"] in (15, 25) and centre(c, ch) for c, ch in zip(cs, chans))
    assert any(c["sf"] not in (0, 5) for c in cs)
    seen = {(ch["scheme"], c["ports"]) for c, ch in zip(cs, chans)}
    assert {("port0", 1), ("txd", 2), ("txd", 4), ("cdd", 2), ("mux1", 2), ("mux2", 2)} <= seen
    assert {c["pmi"] for c, ch in zip(cs, chans) if ch["scheme"] == "mux1"} == {0, 1, 2, 3} and {c["pmi"] for c, ch in zip(cs, chans) if ch["scheme"] == "mux2"} == {1, 2}
    assert {c["fmt"] for c in cs} == {"1A", "1", "2A", "2", "SI"}
    assert {c["fmt"] for c, ch in zip(cs, chans) if None in c["tb"] and ch["scheme"] == "txd"} == {"2A", "2"}      # one block disabled: the fall-back
    assert any(None in c["tb"] and ch["scheme"] == "mux1" for c, ch in zip(cs, chans))
    assert [c["tb"][0] is None for c in cs] == [bool(c.get("gated")) for c in cs] and any(c.get("gated") for c in cs) and any(c.get("swap") for c in cs)
    assert {cw["Qm"] for ch in chans for cw in ch["cw"]} == {2, 4, 6, 8} and any(c.get("t256") for c in cs)
    assert any(len(ch["cw"]) == 2 and ch["cw"][0]["Qm"] != ch["cw"][1]["Qm"] for ch in chans)
    assert any(len(ch["prbs"]) == 1 for ch in chans) and sum(len(ch["prbs"]) == c["prb"] for c, ch in zip(cs, chans)) >= 2
    assert any(c["prb"] % DCI.rbg_size(c["prb"]) and c["prb"] - 1 in ch["prbs"] and c["fmt"] not in ("1A", "SI") for c, ch in zip(cs, chans))   # the short last RBG
    assert {DCI.rbg_size(c["prb"]) for c in cs if c["fmt"] not in ("1A", "SI")} == {1, 2, 3, 4} and {50, 100} <= {c["prb"] for c in cs}
    blocks = [(cw["seg"], t) for ch in chans for cw in ch["cw"] for t in cw["blocks"]]
    assert any(s["C"] == 1 and t["K"] == 40 for s, t in blocks)
    assert any(s["C"] == 3 for s, t in blocks) and CASES[4]["tb"] == [(28, 0)] and CASES[4]["prb"] == 25
    assert any(t["E"] > 3 * 32 * (-(-(t["K"] + 4) // 32)) and len(ch["prbs"]) > 10 for ch in chans for cw in ch["cw"] for t in cw["blocks"])   # E > K_w on many PRBs
    assert {c["tb"][0][1] for c in cs if c["fmt"] == "SI"} == {0, 1, 2, 3} and {c["n1a"] for c in cs if c["fmt"] == "SI"} == {2, 3}
    # every case leaves the decoder something to work with: the code rate stays below 0.9
    for i, ch in enumerate(chans):
        for cw in ch["cw"]:
            assert (len(cw["bits"]) + 24) / cw["G"] < 0.9, (i, len(cw["bits"]), cw["G"])
    # every SI-RNTI version decodes alone: the whole mother code fits
    for c, ch in zip(cs, chans):
        if c["fmt"] == "SI":
            assert ch["cw"][0]["G"] >= 3 * (ch["cw"][0]["blocks"][0]["K"] + 4)


def test_transmit_diversity_pairs_stay_inside_a_prb():
    """36.211 6.3.5 maps transmit-diversity pairs over consecutive available elements; k_pdsch_demod pairs inside a PRB and gives an element without a
    partner zero soft bits.  The two are the same thing on every cell with two or four ports: each PRB has an even number of PDSCH elements in each symbol
    (12, 8, or a half PRB of 6 / 4 next to the PBCH / PSS / SSS), so no pair ever leaves its PRB.  A quadruplet of SFBC-FSTD does (half PRBs hold 6)."""
    quad_leaves = False
    for nprb in (6, 15, 25):
        for ports in (2, 4):
            for cp in (0, 1):
                for sf, cid in ((0, 0), (5, 1), (3, 2)):
                    res = SP.pdsch_res(nprb, ports, cid, cp, sf, 1, range(nprb))
                    cnt = {}
                    for l, k in res:
                        cnt[(l, k // 12)] = cnt.get((l, k // 12), 0) + 1
                    assert all(v % 2 == 0 for v in cnt.values()), (nprb, ports, cp, sf)
                    quad_leaves |= any(v % 4 for v in cnt.values())
    assert quad_leaves


def test_sum_of_block_sizes_is_G_and_re_count_equals_the_oracles():
    for i in range(NCASES):
        p, _, truth, _, _ = case(i)
        ch = truth["pdsch"][0]
        for cw in ch["cw"]:
            assert sum(t["E"] for t in cw["blocks"]) == cw["G"] == len(ch["res"]) * cw["Qm"] == len(cw["f"])
        g = OGrant()
        for n in ch["prbs"]:
            g.prb_idx[0][n] = g.prb_idx[1][n] = 1
        cell = ocell(p)
        assert oracle().o_ra_nof_re(C.byref(cell), p["sf_idx"], p["cfi"], C.byref(g)) == len(ch["res"]), i


# ---------------------------------------------------------------------------------------------------------------------------- the oracle on the streams
def _decode_and_check(i, snr_db=None):
    p, iq, truth, records, dci = case(i, snr_db)
    ow, tr = run_oracle_case(p, iq)
    assert ow.cfi() == p["cfi"], ("SET-UP: CFI", i)
    check_accepted(ow.accepted(), i, dci)
    check_records(parse_pcap(ow.pcap_bytes()), records)
    return p, truth["pdsch"][0], tr


@pytest.mark.parametrize("i", range(NCASES))
def test_pdsch_chain_on_the_spec_transmitter(i):
    p, ch, tr = _decode_and_check(i)
    if CASES[i].get("gated"):
        assert not [j for j in tr if j["rnti"] == ch["rnti"]]
        return
    jobs = matching_jobs(tr, ch, 10 * p["sfn"] + p["sf_idx"])
    assert len(jobs) == 1, ("decode calls with the transmitted parameters", len(jobs), [(hex(j["rnti"]), j["qm"], j["nof_re"]) for j in tr])
    nchk, njudged = check_job(jobs[0], ch, 12 * p["nof_prb"], i)
    assert nchk == sum(cw["seg"]["C"] for cw in ch["cw"]) and njudged == sum(cw["G"] for cw in ch["cw"])
    if CASES[i].get("t256"):    # the table is found by trial: the 64QAM-table attempt comes first and fails
        assert len(tr) == 2 and tr[0]["qm"] != tr[1]["qm"] and not any(cb["ok"] for cb in tr[0]["cbs"])


@pytest.mark.parametrize("i", NOISY)
def test_payloads_survive_awgn(i):
    _decode_and_check(i, NOISY_SNR_DB)


def _block_level(K, F, E, rv, seed):
    """one code block with filler bits through o_rm_turbo_rx_cb and o_turbo_decode_cb: soft bits +-100 from the spec encoder"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2, K).astype(np.uint8)
    c[:F] = SP.NULL
    c[K - 24:] = SP.crc24(np.where(c[:K - 24] == SP.NULL, 0, c[:K - 24]), SP.G_CRC24A)
    d = SP.turbo_encode(c)
    e, src = SP.rate_match(d, E, rv)
    soft = np.where(e == 1, 100, -100).astype(np.int16)
    d3 = np.zeros(3 * (K + 4), dtype=np.int16)
    lib = oracle()
    lib.o_rm_turbo_rx_cb(soft.ctypes.data_as(C.c_void_p), E, K, F, rv, d3.ctypes.data_as(C.c_void_p))
    check_d3(d3, dict(d=d, src=src))
    bits = np.zeros(K, dtype=np.uint8)
    ok = C.c_int(0)
    lib.o_turbo_decode_cb(d3.ctypes.data_as(C.c_void_p), K, 12, C.c_uint32(SP.G_CRC24A), bits.ctypes.data_as(C.c_void_p), C.byref(ok))
    assert ok.value == 1 and np.array_equal(bits, np.where(c == SP.NULL, 0, c))


@pytest.mark.parametrize("K,F,E,rv", [(40, 8, 132 - 16, 0), (1056, 31, 2000, 0), (1056, 31, 2000, 2), (6144, 63, 14000, 3), (512, 1, 3 * 516 + 40, 1)])
def test_filler_bits_at_block_level(K, F, E, rv):
    """no downlink grant reaches F > 0 (module docstring): the place of the filler and <NULL> bits on the oracle's entry points"""
    _block_level(K, F, E, rv, K + rv)

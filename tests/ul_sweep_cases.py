"""Plans that put chosen code blocks (K, F, E, rv) through the production k_rm -> k_turbo path of the uplink entry (Phy.pusch_decode takes explicit grants:
tbs = K - 24 and E = 144 L_prb Qm pick any single block), and their evaluation on the CPU oracle alone.  No GPU here.

Plan A: one single-block grant per turbo block size of 36.212 Table 5.1.3-3 (188), Qm cycling 2 / 4 / 6 / 8 and rv 0 / 2 / 3 / 1, L_prb the valid uplink size
        nearest to a code rate of 0.6 (rv 0) or 0.4 (rv != 0), packed first-fit into 50-PRB subframes.  Every grant has its own gain, tuned on the oracle
        (tune_plan_a, `python tests/ul_sweep_cases.py tune`) so that the block passes after two or more iterations; the tuned table is
        tests/golden/ul_sweep_gains.json.  The plan is run at those gains and once more with every gain lowered by LOWERED_DB.
Plan B: the regimes of the rate de-matcher, chosen by arithmetic: E above the staging cap (un-staged form) next to blocks below it, later blocks of a
        transport block that start 2, 4 and 6 entries past a 16-byte boundary, filler bits punctured and repeated at every rv, a transport block with K- and
        K+ blocks; and two calls of one block each that put the decoder's kmax at its floor (K = 40) and its ceiling (K = 6144).

segment() / blocks_of() restate 36.212 5.1.2 and 5.1.4.1.2 here, so the tests have the block list of a grant without asking product or oracle."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np

from lsn_testlib import (OCell, OPuschGrant, OUci, OUlCfg, TxgUlCell, VALID_UL_PRB, oracle_ul_api, ul_make_subframe)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAINS_JSON = os.path.join(ROOT, "tests", "golden", "ul_sweep_gains.json")
NPRB, N_FFT, CELL_ID, CYCLIC_SHIFT, DELTA_SS = 50, 1024, 101, 3, 5
MAX_ITER = 12
RM_STAGE_CAP = (65536 - 32) // 2     # entries of k_rm's staging area (lsn_launch_rm): a block with E above it is read from global memory
SNR_A = 10.0                         # subframe SNR of plan A: a grant's SNR per resource element is SNR_A + its gain_db
LOWERED_DB = 0.75                    # the second run of plan A: every gain lowered by this much (chosen on the oracle: lowered_counts())
CRC24A, CRC24B = 0x1864CFB, 0x1800063


def _qpp_sizes():
    txt = open(os.path.join(ROOT, "spec", "lte_tables.h")).read()
    m = re.search(r"lsn_qpp_table\[LSN_QPP_NSIZES\]\[3\] = \{(.*?)\};", txt, re.S)
    return [int(x.split(",")[0]) for x in re.findall(r"\{(\d+,\d+,\d+)\}", m.group(1))]


KS = _qpp_sizes()


def segment(tbs):
    """36.212 5.1.2 -> (C, K of every block, F of the first block)"""
    B = tbs + 24
    nC = 1 if B <= 6144 else -(-B // (6144 - 24))
    Bp = B if nC == 1 else B + 24 * nC
    ip = next(i for i, K in enumerate(KS) if nC * K >= Bp)
    Kp = KS[ip]
    if nC == 1:
        return 1, [Kp], Kp - Bp
    Km = KS[ip - 1]
    Cm = (nC * Kp - Bp) // (Kp - Km)
    return nC, [Km] * Cm + [Kp] * (nC - Cm), (nC - Cm) * Kp + Cm * Km - Bp


def blocks_of(g):
    """the code blocks of grant g (no control information, normal cyclic prefix) in transport-block order, 36.212 5.1.4.1.2 with N_L = 1: dict(K, F, E, rv, off =
    where the block's soft bits start in the grant's G = 144 L_prb Qm, nn = entries of its circular buffer that are not <NULL>)"""
    nC, Ks, F = segment(g["tbs"])
    Qm = g["mod"]
    Gp = 144 * g["L_prb"]
    gamma = Gp % nC
    out, off = [], 0
    for r, K in enumerate(Ks):
        E = Qm * (Gp // nC) if r <= nC - gamma - 1 else Qm * -(-Gp // nC)
        Fr = F if r == 0 else 0
        out.append(dict(K=K, F=Fr, E=E, rv=g.get("rv", 0), off=off, nn=3 * (K + 4) - 2 * Fr, crc_b=int(nC > 1)))
        off += E
    assert off == Gp * Qm
    return out


def _grant(i, sf, n_prb, L, Qm, tbs, rv, gain_db=0.0):
    return dict(sf=sf, rnti=1000 + 37 * i, n_dmrs=i % 8, n_prb=n_prb, L_prb=L, mod=Qm, tbs=tbs, rv=rv, gain_db=float(gain_db), phase_rad=(0.7 * i) % 6.28, ta_samples=0.75 * (i % 4))


class _Packer:
    """first fit of contiguous allocations into 50-PRB subframes"""

    def __init__(self):
        self.used = []

    def place(self, L, sf_min=0):
        for sf in range(sf_min, len(self.used)):
            if self.used[sf] + L <= NPRB:
                break
        else:
            self.used.append(0)
            sf = len(self.used) - 1
        n_prb = self.used[sf]
        self.used[sf] += L
        return sf, n_prb


def plan_a_shape(i):
    """block size i of the table -> (K, Qm, rv, L_prb).  Qm changes with every size, rv with every fourth plus one: all sixteen pairs occur"""
    K = KS[i]
    Qm, rv = (2, 4, 6, 8)[i % 4], (0, 2, 3, 1)[(i + i // 4) % 4]
    target = 0.6 if rv == 0 else 0.4
    L = min((n for n in VALID_UL_PRB if n <= NPRB), key=lambda n: (abs(K / (144.0 * n * Qm) - target), n))
    return K, Qm, rv, L


def load_gains():
    with open(GAINS_JSON) as f:
        d = json.load(f)
    assert d["snr_db"] == SNR_A and len(d["gain_db"]) == len(KS)
    return [float(x) for x in d["gain_db"]]


def plan_a(gains=None, lowered=0.0):
    """-> call dict(name, tti0, nsf, snr_db, grants); grant i carries block size KS[i]"""
    gains = load_gains() if gains is None else gains
    pk, grants = _Packer(), []
    for i in range(len(KS)):
        K, Qm, rv, L = plan_a_shape(i)
        sf, n_prb = pk.place(L)
        grants.append(_grant(i, sf, n_prb, L, Qm, K - 24, rv, gains[i] - lowered))
    return dict(name="A-%.2f" % lowered, tti0=1234, nsf=len(pk.used), snr_db=SNR_A, seed=11, grants=grants)


def plan_b():
    """the de-rate-matcher's regimes in one call (the staging area of that launch is at its cap); every grant at 30 dB"""
    pk, grants = _Packer(), []

    def add(L, Qm, tbs, rv, sf_min=0):
        sf, n_prb = pk.place(L, sf_min)
        grants.append(_grant(len(grants), sf, n_prb, L, Qm, tbs, rv))
    # un-staged form: 30 PRB at Qm 8 = 34 560 soft bits for one block of K = 6144 / K = 40 (about 260 repetitions of every entry: the sums clip) / K = 2112 with F = 56
    for tbs in (6120, 16, 2032):
        for rv in range(4):
            add(30, 8, tbs, rv)
    add(27, 8, 6120, 0)        # E = 31 104: just under the cap, staged
    # filler bits F = 8 / 24 / 56, punctured (E < nn) and repeated (E > nn), at every rv; they share the subframes of the blocks above where they fit
    for rv in range(4):
        for Qm, tbs, Ls in ((2, 512, (4, 8)), (4, 1040, (4, 8)), (6, 2032, (5, 10))):
            for L in Ls:
                add(L, Qm, tbs, rv)
    # seven code blocks (four of K-, three of K+, F = 16 on the first) at Qm 6 on 50 PRB: E = 6168 x 3, 6174 x 4 - the later blocks start 6, 4 and 2 entries past a 16-byte boundary
    for rv in (0, 2):
        add(50, 6, 36720, rv)
    return dict(name="B", tti0=4321, nsf=len(pk.used), snr_db=30.0, seed=12, grants=grants)


def plan_single(K):
    """a call that decodes one block: the decoder launch's kmax is this K (40: the LDS floor of 512, 6144: the ceiling)"""
    L, Qm = (1, 2) if K == 40 else (12, 6)
    return dict(name="K%d" % K, tti0=777, nsf=1, snr_db=30.0, seed=13, grants=[_grant(5, 0, 7, L, Qm, K - 24, 0)])


def realise(call):
    """-> (iq complex64 [nsf, 15 N], payload bytes per grant)"""
    ucell = TxgUlCell(NPRB, CELL_ID, CYCLIC_SHIFT, DELTA_SS, 0, 0)
    iq = np.zeros((call["nsf"], 15 * N_FFT), dtype=np.complex64)
    payloads = [None] * len(call["grants"])
    for sf in range(call["nsf"]):
        idx = [i for i, g in enumerate(call["grants"]) if g["sf"] == sf]
        iq[sf], pl = ul_make_subframe(ucell, call["tti0"] + sf, [call["grants"][i] for i in idx], snr_db=call["snr_db"], seed=call["seed"] * 100 + sf)
        for i, p in zip(idx, pl):
            payloads[i] = p
    return iq, payloads


def oracle_eval(call, iq, whole=True):
    """the oracle on every grant of the call: o_ul_fft, o_pusch_demod_uci, then per block o_rm_turbo_rx_cb and o_turbo_decode_cb on the oracle's own soft bits;
    whole: also o_pusch_decode_uci (verdict, iteration count, SNR estimate and payload of the transport block).
    -> (grids, per grant dict(e, blocks=[dict(K, F, E, rv, off, nn, d3, ok, iters)], crc, iters, snr_bits, payload))"""
    o = oracle_ul_api()
    ocell, ucfg = OCell(NPRB, 1, CELL_ID, 1), OUlCfg(CYCLIC_SHIFT, DELTA_SS, 0, 0, 0)
    grids = []
    for sf in range(call["nsf"]):
        g = np.zeros(14 * 12 * NPRB, dtype=np.complex64)
        o.o_ul_fft(C.byref(ocell), iq[sf].ctypes.data, g.ctypes.data)
        grids.append(g)
    res = []
    for g in call["grants"]:
        og, uci = OPuschGrant(g["L_prb"], g["n_prb"], 0, g["mod"], g["tbs"], g["rv"], 0, 0), OUci(0, 0, 0)
        sf_idx = (call["tti0"] + g["sf"]) % 10
        e = np.zeros(144 * g["L_prb"] * g["mod"], dtype=np.int16)
        assert o.o_pusch_demod_uci(C.byref(ocell), C.byref(ucfg), sf_idx, g["rnti"], C.byref(og), g["n_dmrs"], C.byref(uci), grids[g["sf"]].ctypes.data,
                                   e.ctypes.data, None, None) == 0
        blocks = []
        for b in blocks_of(g):
            K = b["K"]
            d3 = np.zeros((3, K + 4), dtype=np.int16)
            eb = np.ascontiguousarray(e[b["off"]:b["off"] + b["E"]])
            o.o_rm_turbo_rx_cb(eb.ctypes.data, b["E"], K, b["F"], b["rv"], d3.ctypes.data)
            bits, ok = np.zeros(K, dtype=np.uint8), C.c_int(0)
            its = o.o_turbo_decode_cb(d3.ctypes.data, K, MAX_ITER, CRC24B if b["crc_b"] else CRC24A, bits.ctypes.data, C.byref(ok))
            blocks.append(dict(b, d3=d3, ok=ok.value, iters=its))
        r = dict(e=e, blocks=blocks)
        if whole:
            out = np.zeros(g["tbs"] // 8 + 8, dtype=np.uint8)
            its, snr = C.c_int(0), C.c_float(0)
            r["crc"] = o.o_pusch_decode_uci(C.byref(ocell), C.byref(ucfg), sf_idx, g["rnti"], C.byref(og), g["n_dmrs"], C.byref(uci), grids[g["sf"]].ctypes.data,
                                            MAX_ITER, out.ctypes.data, C.byref(its), C.byref(snr))
            r["iters"], r["snr_bits"], r["payload"] = its.value, int(np.float32(snr.value).view(np.uint32)), bytes(out[:g["tbs"] // 8])
        res.append(r)
    return grids, res


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """(call, iq, payloads, grids, oracle results) of the plan `name` - computed once, shared by the tests of a run and left unchanged by them.
    name: "A" (tuned gains), "A-low" (lowered by LOWERED_DB), "B", "K40", "K6144" """
    call = {"A": plan_a, "A-low": lambda: plan_a(lowered=LOWERED_DB), "B": plan_b, "K40": lambda: plan_single(40), "K6144": lambda: plan_single(6144)}[name]()
    iq, payloads = realise(call)
    iq.setflags(write=False)
    grids, res = oracle_eval(call, iq)
    return call, iq, payloads, grids, res


# ---- tuning (a tool, not run by the tests): python tests/ul_sweep_cases.py tune | lowered

def tune_plan_a(rounds=16, log=print):
    """per grant: +-1 dB for eight rounds, then +-0.5 dB - up when the block fails or needs more than 8 iterations, down when it needs fewer than 3; the gain kept
    is the one at which it passed with the most iterations (at most 10, which leaves two to the limit), else the lowest at which it passed"""
    gains = [{2: -7.0, 4: -2.0, 6: 3.0, 8: 8.0}[plan_a_shape(i)[1]] - (0.0 if plan_a_shape(i)[2] == 0 else 2.0) for i in range(len(KS))]
    best = [None] * len(KS)      # (score, gain)

    def score(b, gain):
        if not b["ok"]:
            return None
        return (b["iters"] if 2 <= b["iters"] <= 10 else 0, -gain)

    def run(gains):
        call = plan_a(gains)
        iq, _ = realise(call)
        return [r["blocks"][0] for r in oracle_eval(call, iq, whole=False)[1]]
    for rnd in range(rounds):
        step = 1.0 if rnd < rounds // 2 else 0.5
        bl = run(gains)
        for i, b in enumerate(bl):
            s = score(b, gains[i])
            if s is not None and (best[i] is None or s > best[i][0]):
                best[i] = (s, gains[i])
            if not b["ok"] or b["iters"] > 8:
                gains[i] += step
            elif b["iters"] < 3:
                gains[i] -= step
        log("round %d: pass %d, >= 2 iterations %d, >= 3 %d" % (rnd, sum(b["ok"] for b in bl), sum(b["ok"] and b["iters"] >= 2 for b in bl), sum(b["ok"] and b["iters"] >= 3 for b in bl)))
    gains = [best[i][1] if best[i] else gains[i] for i in range(len(KS))]
    for _ in range(6):           # the table as a whole (a grant's samples are rounded to float32 together with its neighbours'): lift what fails now
        bl = run(gains)
        bad = [i for i, b in enumerate(bl) if not b["ok"] or b["iters"] > 10]
        log("final: pass %d, >= 2 iterations %d, >= 3 %d, lifted %s" % (sum(b["ok"] for b in bl), sum(b["ok"] and b["iters"] >= 2 for b in bl), sum(b["ok"] and b["iters"] >= 3 for b in bl), bad))
        if not bad:
            break
        for i in bad:
            gains[i] += 0.5
    return gains


def lowered_counts(step):
    call = plan_a(lowered=step)
    iq, _ = realise(call)
    bl = [r["blocks"][0] for r in oracle_eval(call, iq, whole=False)[1]]
    return sum(b["ok"] for b in bl), sum((not b["ok"]) and b["iters"] == MAX_ITER for b in bl)


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["tune"]:
        g = tune_plan_a()
        with open(GAINS_JSON, "w") as f:
            json.dump(dict(snr_db=SNR_A, gain_db=g), f)
            f.write("\n")
    for s in (0.25, 0.5, 0.75, 1.0, 1.5):
        print("lowered by %.2f dB: pass %d, fail at the iteration limit %d" % ((s,) + lowered_counts(s)))

"""What the GPU sweep of k_rm and k_turbo (test_gpu_ul_sweep.py) relies on, asserted on the plans and the CPU oracle alone (ul_sweep_cases.py): plan A visits every
turbo block size, every window count and every W % 8 residue of the decoder, at gains where the oracle needs several iterations (and, lowered, where it gives
up on many); plan B holds every regime of the rate de-matcher, each stated as a predicate on (K, F, E, rv, start of the block modulo 8, E against the staging cap
and the circular buffer's length).  No GPU."""
import collections

import numpy as np

import ltesniffer_amd as la
from lsn_testlib import VALID_UL_PRB, hosttest
from ul_sweep_cases import KS, LOWERED_DB, MAX_ITER, NPRB, RM_STAGE_CAP, blocks_of, evaluated, plan_a, plan_a_shape, plan_b, plan_single, segment


def _fits(call):
    """every grant on valid, disjoint PRBs of its subframe"""
    used = collections.defaultdict(set)
    for g in call["grants"]:
        prbs = set(range(g["n_prb"], g["n_prb"] + g["L_prb"]))
        assert g["L_prb"] in VALID_UL_PRB and max(prbs) < NPRB and 0 <= g["sf"] < call["nsf"] and not (prbs & used[g["sf"]]), g
        assert g["tbs"] % 8 == 0 and g["mod"] in (2, 4, 6, 8) and 0 <= g["rv"] < 4
        used[g["sf"]] |= prbs


def test_segmentation_restated_here_is_the_host_logic():
    import ctypes as C
    h = hosttest()
    seg = (C.c_int * 6)()
    for tbs in [K - 24 for K in KS] + [512, 1040, 2032, 6120, 6128, 36720, 12216, 75376]:
        assert h.lsnh_cbsegm(tbs, seg) == 0
        nC, Cp, Cm, Kp, Km, F = list(seg)
        assert segment(tbs) == (nC, [Km] * Cm + [Kp] * Cp, F), tbs


def test_unpacking_inverts_the_layout_k_rm_writes():
    """la.unpack_rm_words (Phy.stage_c_jobs and Phy.tap_ul_cbs read k_rm's output through it) on words packed here the way stage_c.hip states the layout: word t holds
    trellis position x = (t % P) * W + t // P, systematic | parity 1 << 10 | parity 2 << 20 in ten bits each, words K + 4 s + j the termination value j of stream s"""
    rng = np.random.default_rng(5)
    for K in KS:
        P = la.turbo_nwin(K)
        W = K // P
        d3 = rng.integers(-511, 512, size=(3, K + 4)).astype(np.int16)
        d3[:, :3] = [[-511, 511, 0]] * 3
        w = np.zeros(K + 12, dtype=np.uint32)
        t = np.arange(K)
        f = d3[:, (t % P) * W + t // P].astype(np.int64) & 0x3FF
        w[:K] = f[0] | (f[1] << 10) | (f[2] << 20)
        for s in range(3):
            w[K + 4 * s:K + 4 * s + 4] = d3[s, K:].astype(np.int32).view(np.uint32)
        got = la.unpack_rm_words(w, K)
        assert got.dtype == np.int16 and np.array_equal(got, d3), K


def test_plan_a_names_every_block_size_window_count_and_residue():
    h = hosttest()
    call = plan_a()
    _fits(call)
    assert len(KS) == 188 and call["nsf"] <= 32
    blocks = [blocks_of(g) for g in call["grants"]]
    assert all(len(b) == 1 and b[0]["F"] == 0 for b in blocks)
    assert sorted(b[0]["K"] for b in blocks) == KS                         # all 188 sizes, once each
    nwin = {la.turbo_nwin(K) for K in KS}
    assert {h.lsnh_turbo_nwin(K) for K in KS} == nwin and min(nwin) == 1 and max(nwin) == 128
    assert {la.turbo_nwin(b[0]["K"]) for b in blocks} == nwin               # every P the decoder uses
    assert {(b[0]["K"] // la.turbo_nwin(b[0]["K"])) % 8 for b in blocks} == set(range(8))   # every head length of the per-window CRC weight
    assert {h.lsnh_turbo_two_wave_class(b[0]["K"]) for b in blocks} == {0, 1}
    assert {(g["mod"], g["rv"]) for g in call["grants"]} == {(q, r) for q in (2, 4, 6, 8) for r in range(4)}
    for i, g in enumerate(call["grants"]):                                    # the size nearest to a code rate of 0.6 / 0.4 among the valid ones
        K, Qm, rv, L = plan_a_shape(i)
        target = 0.6 if rv == 0 else 0.4
        assert (g["L_prb"], g["mod"], g["rv"], g["tbs"]) == (L, Qm, rv, K - 24)
        assert all(abs(K / (144.0 * L * Qm) - target) <= abs(K / (144.0 * n * Qm) - target) for n in VALID_UL_PRB if n <= NPRB)
    # both forms of the de-rate-matcher's inner step occur: punctured and repeated blocks
    assert any(b[0]["E"] < b[0]["nn"] for b in blocks) and any(b[0]["E"] > b[0]["nn"] for b in blocks)


def test_plan_a_at_the_tuned_gains_makes_the_decoder_iterate():
    call, _, payloads, _, res = evaluated("A")
    bl = [r["blocks"][0] for r in res]
    n_pass = sum(b["ok"] for b in bl)
    n2 = sum(b["ok"] and b["iters"] >= 2 for b in bl)
    n3 = sum(b["ok"] and b["iters"] >= 3 for b in bl)
    print("plan A, tuned gains: pass %d, >= 2 iterations %d, >= 3 iterations %d, histogram %s" % (n_pass, n2, n3, sorted(collections.Counter(b["iters"] for b in bl).items())))
    assert n_pass == 188                                                      # every size passes ...
    assert n2 >= 186 and n3 >= 185                                            # ... nearly all of them only after the extrinsic values went round (what the tuner reached)
    assert all(b["iters"] <= MAX_ITER - 2 for b in bl)                        # two iterations to spare
    for r, b, pl in zip(res, bl, payloads):                                   # the transport-block view of the same decode
        assert (r["crc"], r["iters"]) == (b["ok"], b["iters"]) and r["payload"] == pl


def test_plan_a_lowered_has_blocks_on_both_sides_of_the_limit():
    _, _, payloads, _, res = evaluated("A-low")
    bl = [r["blocks"][0] for r in res]
    n_fail = sum((not b["ok"]) and b["iters"] == MAX_ITER for b in bl)
    n_pass = sum(b["ok"] for b in bl)
    print("plan A, gains lowered by %.2f dB: pass %d, fail at %d iterations %d" % (LOWERED_DB, n_pass, MAX_ITER, n_fail))
    assert n_fail >= 30 and n_pass >= 30 and n_fail + n_pass == 188
    assert all(r["payload"] == pl for r, b, pl in zip(res, bl, payloads) if b["ok"])


def _plan_b_blocks():
    call = plan_b()
    out = []
    for g in call["grants"]:
        bl = blocks_of(g)
        for q, b in enumerate(bl):
            out.append(dict(b, q=q, C=len(bl), skew=b["off"] % 8, grant=g))     # (a grant's soft bits start on a 16-byte boundary: b["off"] % 8 is the block's own)
    return call, out


def test_plan_b_holds_every_regime_of_the_de_rate_matcher():
    call, bl = _plan_b_blocks()
    _fits(call)
    assert call["nsf"] <= 25 and len(bl) <= 64

    def has(pred):
        return any(pred(b) for b in bl)
    # one call: its staging area is capped, and blocks on both sides of the cap are in it
    assert max(b["E"] for b in bl) > RM_STAGE_CAP
    for rv in range(4):
        assert has(lambda b: b["E"] > RM_STAGE_CAP and b["K"] == 6144 and b["rv"] == rv)                                  # un-staged, the largest block
        assert has(lambda b: b["E"] > RM_STAGE_CAP and b["K"] == 40 and b["E"] >= 250 * b["nn"] and b["rv"] == rv)        # un-staged, hundreds of repetitions: the sum clips
        assert has(lambda b: b["E"] > RM_STAGE_CAP and b["F"] == 56 and b["rv"] == rv)                                    # un-staged with filler
    assert has(lambda b: RM_STAGE_CAP - 2048 < b["E"] <= RM_STAGE_CAP)                                                      # staged, just under the cap
    assert has(lambda b: b["E"] <= b["nn"] and b["E"] <= RM_STAGE_CAP) and has(lambda b: b["nn"] < b["E"] <= RM_STAGE_CAP)  # `single` and `staged` forms
    for skew in (2, 4, 6):                                                                                                 # staging starts off a 16-byte boundary
        assert has(lambda b: b["C"] > 1 and b["q"] > 0 and b["skew"] == skew)
    assert not has(lambda b: b["skew"] % 2)                                                                                # (E is a multiple of Qm: never odd)
    for F in (8, 24, 56):
        for rv in range(4):
            assert has(lambda b: b["C"] == 1 and b["F"] == F and b["rv"] == rv and b["E"] < b["nn"])                        # filler, punctured
            assert has(lambda b: b["C"] == 1 and b["F"] == F and b["rv"] == rv and b["nn"] < b["E"] <= RM_STAGE_CAP)        # filler, repeated
    multi = [b for b in bl if b["C"] > 1]
    assert any(b["q"] == 0 and b["F"] > 0 for b in multi) and len({b["K"] for b in multi if b["grant"] is multi[0]["grant"]}) == 2   # K- and K+ in one transport block
    # the two calls of one block: kmax of the decoder launch at its floor and its ceiling
    for K in (40, 6144):
        c = plan_single(K)
        _fits(c)
        assert len(c["grants"]) == 1 and [b["K"] for b in blocks_of(c["grants"][0])] == [K]


def test_plan_b_decodes_on_the_oracle():
    """30 dB: what plan B sends is meant to come through (a transport block at code rate 0.85 and rv 2 alone may not); the verdicts themselves are the GPU test's to compare"""
    for name in ("B", "K40", "K6144"):
        call, _, payloads, _, res = evaluated(name)
        for g, r, pl in zip(call["grants"], res, payloads):
            assert r["iters"] == sum(b["iters"] for b in r["blocks"]) and (not r["crc"] or all(b["ok"] for b in r["blocks"]))
            if len(r["blocks"]) == 1 or g["rv"] == 0:
                assert r["crc"] == 1 and r["payload"] == pl, (name, g)
    _, _, _, _, res = evaluated("B")
    assert any(np.abs(b["d3"][:, :b["K"]]).min() == 511 for r in res for b in r["blocks"] if b["K"] == 40)   # every sum of the K = 40 blocks clipped

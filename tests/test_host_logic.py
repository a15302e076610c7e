"""CPU tests (no GPU): the product's HIP-free host logic (DCI sizes/unpack, grants, search space, FALCON search, code
block segmentation, rate-matcher index arithmetic) against the oracle's independent restatement."""
import ctypes as C
import subprocess
import os

import numpy as np
import pytest

from lsn_testlib import (LsnCand, OCbSegm, OCell, OGrant, OracleWorker, TxGen, candidate_table, hosttest, oracle, scenario, ROOT,
                         MAX_LOC, MAX_SIZES, CCE_STRIDE)


def test_rm_index_closed_form():
    hosttest()
    out = subprocess.check_output([os.path.join(ROOT, "tests", "native", "_build", "test_rm_index")]).decode()
    assert out.startswith("OK")


@pytest.mark.parametrize("nprb,ports", [(6, 1), (15, 2), (25, 1), (25, 2), (50, 1), (50, 2), (75, 1), (75, 2), (100, 1), (100, 2),
                                        (6, 4), (15, 4), (25, 4), (50, 4), (75, 4), (100, 4)])
def test_dci_sizes(nprb, ports):
    h, o = hosttest(), oracle()
    cell = OCell(nprb, ports, 1, 1)
    for f in range(9):
        assert h.lsnh_dci_format_sizeof(nprb, ports, f) == o.o_dci_format_sizeof(C.byref(cell), f), f


def test_search_space_closed_form_vs_enumeration():
    h, o = hosttest(), oracle()
    rng = np.random.default_rng(5)
    for cces in ([20, 54, 87], [10, 26, 43], [2, 5, 9], [4, 12, 21]):
        arr = (C.c_uint32 * 3)(*cces)
        rntis = list(rng.integers(0, 65536, 400)) + [0, 1, 2, 9, 10, 11, 0xFFF3, 0xFFF4, 0xFFFC, 0xFFFD, 0xFFFE, 0xFFFF]
        for cfi in (1, 2, 3):
            n = cces[cfi - 1]
            for rnti in rntis:
                for l in range(4):
                    L = 1 << l
                    for ncce in range(0, min(n, 84) - L + 1, L):
                        sf = int(rng.integers(0, 10))
                        a = h.lsnh_validate_location(arr, cfi, ncce, l, sf, int(rnti))
                        b = o.o_validate_location(n, ncce, l, sf, int(rnti))
                        assert a == b, (cces, cfi, ncce, l, sf, rnti, a, b)
                        assert a == h.lsnh_validate_location_enum(n, ncce, l, sf, int(rnti))


def _oracle_grant_api():
    o = oracle()
    o.o_dci_unpack_dl.argtypes = [C.POINTER(OCell), C.c_void_p, C.c_uint32, C.c_int, C.c_uint16, C.c_void_p]
    o.o_ra_dl_dci_to_grant.argtypes = [C.POINTER(OCell), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(OGrant)]
    o.o_config_mimo.argtypes = [C.POINTER(OCell), C.c_int, C.c_void_p, C.POINTER(OGrant)]
    o.o_dci_unpack_ul.argtypes = [C.POINTER(OCell), C.c_void_p, C.c_uint32, C.c_uint16, C.c_void_p]
    o.o_ra_ul_dci_to_grant.argtypes = [C.POINTER(OCell), C.c_void_p, C.c_void_p]
    return o


@pytest.mark.parametrize("nprb,ports", [(100, 2), (75, 2), (50, 1), (25, 2), (6, 1), (15, 2), (100, 4), (25, 4), (6, 4)])
def test_dl_grants_random_payloads(nprb, ports):
    """random DCI payloads of every DL format -> identical unpack verdict, PRB set, TBS/modulation, nof_re, MIMO config"""
    h, o = hosttest(), _oracle_grant_api()
    rng = np.random.default_rng(nprb * 10 + ports)
    cell = OCell(nprb, ports, 3, 1)
    dci = (C.c_uint8 * 512)()
    n_ok = 0
    for it in range(1500):
        fmt = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8]))
        nb = h.lsnh_dci_format_sizeof(nprb, ports, fmt)
        payload = rng.integers(0, 2, nb).astype(np.uint8)
        if fmt == 2:
            payload[0] = 1
        rnti = int(rng.choice([0xFFFF, 0xFFFE, 2, 5, 0x46, 0x1234, int(rng.integers(11, 0xFFF3))]))
        sf_idx, cfi, alt = int(rng.integers(0, 10)), int(rng.integers(1, 4)), int(rng.integers(0, 2))
        C.memset(dci, 0, 512)
        g_o, g_h = OGrant(), OGrant()
        dci_view = (C.c_uint32 * 4).from_buffer(dci)
        u_ok = o.o_dci_unpack_dl(C.byref(cell), payload.ctypes.data, nb, fmt, rnti, dci) == 0
        r_o = 0
        if u_ok:
            r_o = 1
            if o.o_ra_dl_dci_to_grant(C.byref(cell), sf_idx, cfi, alt, dci, C.byref(g_o)) == 0:
                r_o |= 2
                r_o |= o.o_config_mimo(C.byref(cell), fmt, dci, C.byref(g_o)) << 8
        r_h = h.lsnh_dl_grant(nprb, ports, 3, sf_idx, cfi, alt, payload.ctypes.data, nb, fmt, rnti, 1, C.byref(g_h))
        assert r_h == r_o, (fmt, rnti, r_h, r_o)
        if r_o & 2:
            n_ok += 1
            assert bytes(g_h) == bytes(g_o), (fmt, rnti, sf_idx, cfi, alt)
    assert n_ok > 300


def test_ul_grants_random_payloads():
    h, o = hosttest(), _oracle_grant_api()
    rng = np.random.default_rng(9)
    for nprb in (25, 50, 75, 100):
        cell = OCell(nprb, 2, 1, 1)
        nb = h.lsnh_dci_format_sizeof(nprb, 2, 0)
        for it in range(500):
            payload = rng.integers(0, 2, nb).astype(np.uint8)
            payload[0] = 0
            dci = (C.c_uint8 * 256)()
            og = (C.c_uint32 * 8)()
            hg = (C.c_uint32 * 6)()
            r_o = 0
            if o.o_dci_unpack_ul(C.byref(cell), payload.ctypes.data, nb, 0x100, dci) == 0:
                r_o = 1
                if o.o_ra_ul_dci_to_grant(C.byref(cell), dci, og) == 0:
                    r_o = 3
            r_h = h.lsnh_ul_grant(nprb, 2, payload.ctypes.data, nb, 0x100, hg)
            assert r_h == r_o
            if r_o == 3:  # o_pusch_grant_t {L_prb, n_prb, mcs_idx, mod, tbs, rv}
                assert list(hg) == list(og)[:6]


def test_ul_grants_with_frequency_hopping_offsets():
    """DCI 0 with the hopping flag: hop bits (36.213 Tables 8.4-1/2), type-1 second-slot position for several pusch-HoppingOffset values,
    type 2 flagged - product == oracle on random payloads, and a hand-computed case"""
    h, o = hosttest(), _oracle_grant_api()
    h.lsnh_ul_grant_hop.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint16, C.c_void_p]
    rng = np.random.default_rng(19)
    seen = set()
    for nprb in (25, 50, 100):
        nb = h.lsnh_dci_format_sizeof(nprb, 2, 0)
        for off in (0, 3, 8, 20):
            cell = OCell(nprb, 2, 1, 1, off)
            for it in range(400):
                payload = rng.integers(0, 2, nb).astype(np.uint8)
                payload[0] = 0
                payload[1] = 1  # hopping flag
                dci = (C.c_uint8 * 256)()
                og = (C.c_uint32 * 8)()
                hg = (C.c_uint32 * 8)()
                r_o = 0
                if o.o_dci_unpack_ul(C.byref(cell), payload.ctypes.data, nb, 0x100, dci) == 0:
                    r_o = 1
                    if o.o_ra_ul_dci_to_grant(C.byref(cell), dci, og) == 0:
                        r_o = 3
                assert h.lsnh_ul_grant_hop(nprb, 2, off, payload.ctypes.data, nb, 0x100, hg) == r_o
                if r_o == 3:
                    assert list(hg) == list(og)
                    seen.add((nprb, int(og[7])))
                    if og[7] == 1:
                        assert og[6] + og[0] <= nprb and og[6] != og[1] or og[0] == 0
    assert {(25, 1), (25, 2), (100, 1), (100, 2)} <= seen
    # 100 PRB, offset 10: n_rb_pusch = 90; hop bits 10 (= +N/2), L = 4 at PRB 12 -> slot 1 at (45 + 12) % 90 = 57
    nb = h.lsnh_dci_format_sizeof(100, 2, 0)
    riv = 100 * (4 - 1) + 12
    bits = [0, 1, 1, 0] + [int(b) for b in format(riv, "011b")] + [0] * (nb - 15)
    hg = (C.c_uint32 * 8)()
    pl = np.array(bits, dtype=np.uint8)
    assert h.lsnh_ul_grant_hop(100, 2, 10, pl.ctypes.data, nb, 0x100, hg) == 3 and (hg[0], hg[1], hg[6], hg[7]) == (4, 12, 57, 1)


def test_cbsegm_all_tbs():
    h, o = hosttest(), oracle()
    Seg = OCbSegm
    seen = set()
    for itbs in range(0, 34):
        for nprb in range(1, 111):
            seen.add(o.o_tbs_from_idx(itbs, nprb))
    seen.discard(-1)
    assert len(seen) > 150
    for tbs in sorted(seen):
        s = Seg()
        out = (C.c_int * 6)()
        ro, rh = o.o_cbsegm(C.byref(s), tbs), h.lsnh_cbsegm(tbs, out)
        assert (ro == 0) == (rh == 0)
        if ro == 0:
            assert list(out) == [s.C, s.Cp, s.Cm, s.Kp, s.Km, s.F], tbs


def test_tb_code_block_descriptors():
    """tb_code_blocks (the descriptors runJobs and puschDecodeGrid hand to k_rm / k_turbo) against 36.212 5.1.4.1.2 written out here: G' = G / (N_L Q_m),
    gamma = G' mod C, blocks 0 .. C - gamma - 1 get N_L Q_m floor(G' / C) bits and the rest the ceiling; K, F and the payload bytes from lsnh_cbsegm.  Every size of
    the product's TBS table, Qm 2 / 4 / 6 / 8, one and two layers, G = N_L Q_m n_re with gamma = 0, gamma != 0 and fewer symbols than code blocks."""
    h = hosttest()
    sizes = {h.lsnh_tbs_from_idx(i, n) for i in range(0, 34) for n in range(1, 111)}
    sizes.discard(-1)
    sizes.discard(0)
    assert len(sizes) > 150
    NODEP, E0, O0, NBEFORE = 0xFFFFFFFF, 4096, 160, 7
    out, pay, seg = (C.c_uint32 * (7 * 32))(), C.c_uint32(), (C.c_int * 6)()
    multi = with_gamma = starved = 0
    for tbs in sorted(sizes):
        assert h.lsnh_cbsegm(tbs, seg) == 0
        nC, Cp, Cm, Kp, Km, F = list(seg)
        assert 1 <= nC <= 32 and Cp + Cm == nC
        K = [Km if q < Cm else Kp for q in range(nC)]
        Fq = [F if q == 0 else 0 for q in range(nC)]
        nbytes = [(K[q] - Fq[q] - (24 if nC > 1 else 0)) // 8 for q in range(nC)]
        assert sum(nbytes) == (tbs + 24) // 8
        for n_re in sorted({150 * nC, 150 * nC + 1, 97 * nC + nC - 1, max(1, nC - 1)}):
            for Qm in (2, 4, 6, 8):
                for NL in (1, 2):
                    G = NL * Qm * n_re
                    Gp = G // (NL * Qm)
                    gamma = Gp % nC
                    E = [NL * Qm * (Gp // nC) if q <= nC - gamma - 1 else NL * Qm * -(-Gp // nC) for q in range(nC)]
                    assert sum(E) == G
                    multi += nC > 1
                    with_gamma += gamma != 0
                    starved += Gp < nC
                    for dep_first in (0, 1):
                        assert h.lsnh_tb_code_blocks(tbs, G, Qm, NL, E0, O0, dep_first, NBEFORE, out, 32, C.byref(pay)) == nC
                        got = [list(out[7 * q:7 * q + 7]) for q in range(nC)]
                        exp = [[K[q], Fq[q], E[q], E0 + sum(E[:q]), O0 + sum(nbytes[:q]), nbytes[q],
                                NBEFORE if (dep_first and q > 0) else NODEP] for q in range(nC)]
                        assert got == exp, (tbs, G, Qm, NL, dep_first)
                        assert sum(g[2] for g in got) == G
                        assert pay.value == (sum(nbytes) + 15) // 16 * 16
    assert multi and with_gamma and starved


def _crc24a_rem(data):
    """the bytes as a polynomial (first bit = highest power) mod g_CRC24A, no extra shift: what k_turbo reports per code block as rem_a"""
    reg = 0
    for byte in data:
        for i in range(7, -1, -1):
            reg = (reg << 1) | ((byte >> i) & 1)
            if reg & 0x1000000:
                reg ^= 0x1864CFB
    return reg


def test_tb_verdict():
    """TbVerdict (the transport-block verdict of runJobs, puschDecodeGrid and the two HARQ paths) on random payloads of 1 .. 13 code blocks with a CRC24A
    attached by a Python CRC: passes on the clean payload; fails on one flipped bit, one failed block, a truncated last block and the all-zero payload; its
    remainder is the Python CRC of the whole byte string in every case.  The two identities the carried-shift form rests on: a * 1 mod g == a for a < 2^24."""
    h = hosttest()
    rng = np.random.default_rng(24)
    for a in [0, 1, 2, 0x800000, 0xFFFFFF, 0x864CFB] + [int(x) for x in rng.integers(0, 1 << 24, 200)]:
        assert h.lsnh_crc24a_mulmod(a, 1) == a and h.lsnh_crc24a_mulmod(1, a) == a
    out3 = (C.c_uint64 * 3)()

    def verdict(blocks, ok, tbs):
        n = len(blocks)
        pl = np.frombuffer(b"".join(blocks) + bytes(16), dtype=np.uint8).copy()   # (the engine's payload arenas are padded too)
        rem_a = np.array([_crc24a_rem(b) for b in blocks], dtype=np.uint32)
        assert all(int(r) < (1 << 24) for r in rem_a)
        nb = np.array([len(b) for b in blocks], dtype=np.uint32)
        okv = np.array(ok, dtype=np.uint8)
        r = h.lsnh_tb_verdict(n, okv.ctypes.data, rem_a.ctypes.data, nb.ctypes.data, pl.ctypes.data, tbs, out3)
        assert out3[0] == (1 if all(ok) else 0)
        assert out3[1] == _crc24a_rem(b"".join(blocks))
        assert out3[2] == 8 * sum(len(b) for b in blocks)
        # tb_verdict (the helper runJobs and puschDecodeGrid call) on the same blocks as LsnCbRes / LsnCbDev arrays: the same verdict, and the iteration sum
        iters = rng.integers(0, 13, n).astype(np.uint32)
        out4 = (C.c_uint64 * 4)()
        assert h.lsnh_tb_verdict_blocks(n, okv.ctypes.data, rem_a.ctypes.data, iters.ctypes.data, nb.ctypes.data, pl.ctypes.data, tbs, out4) == r
        assert list(out4) == list(out3) + [int(iters.sum())]
        return r

    def split(data, lens):
        o, res = 0, []
        for n in lens:
            res.append(data[o:o + n])
            o += n
        assert o == len(data)
        return res

    for trial in range(60):
        n = trial % 13 + 1
        lens = [int(x) for x in rng.integers(5, 769, n)]
        lens[0] = max(5, lens[0] - int(rng.integers(0, 4)))
        data = bytes(rng.integers(0, 256, sum(lens) - 3, dtype=np.uint8))
        if not any(data):
            data = b"\x01" + data[1:]
        par = _crc24a_rem(data + bytes(3))
        assert par != 0
        whole = data + par.to_bytes(3, "big")
        tbs = 8 * len(data)
        assert _crc24a_rem(whole) == 0
        assert verdict(split(whole, lens), [1] * n, tbs) == 1
        bit = int(rng.integers(0, 8 * len(whole)))
        flipped = bytearray(whole)
        flipped[bit // 8] ^= 0x80 >> (bit % 8)
        assert verdict(split(bytes(flipped), lens), [1] * n, tbs) == 0 and out3[1] != 0
        bad = [1] * n
        bad[int(rng.integers(0, n))] = 0
        assert verdict(split(whole, lens), bad, tbs) == 0 and out3[1] == 0
        cut = int(rng.integers(1, 4))
        assert verdict(split(whole[:-cut], lens[:-1] + [lens[-1] - cut]), [1] * n, tbs) == 0
        assert verdict(split(bytes(len(whole)), lens), [1] * n, tbs) == 0 and out3[1] == 0 and out3[2] == tbs + 24


NODEP = 0xFFFFFFFF
LEGAL_K = list(range(40, 512, 8)) + list(range(512, 1024, 16)) + list(range(1024, 2048, 32)) + list(range(2048, 6145, 64))   # 36.212 Table 5.1.3-3


def _packed_order_sets():
    """(K, dep) lists for the packed launch order: the named edge cases, then random sets of 0 .. 400 blocks of the 188 legal sizes"""
    h = hosttest()
    kmax = h.lsnh_turbo_pair_kmax()
    below, above = max(k for k in LEGAL_K if k <= kmax), min(k for k in LEGAL_K if k > kmax)
    pairable = [k for k in LEGAL_K if k <= kmax and h.lsnh_turbo_nwin(k) <= 64]
    rng = np.random.default_rng(2752)
    sets = [([], []), ([below], [NODEP]), ([6144], [NODEP]),
            (LEGAL_K, [NODEP] * 188),                                          # all independent
            (LEGAL_K[::-1], [NODEP] + [0] * 187),                              # all but one dependent
            ([40, 6144, 40, 6144, below, above, below, above] * 2, [NODEP, NODEP, 0, 1] * 4),   # equal K, the smallest and the largest, both sides of the limit
            (pairable[:3] + [6144], [NODEP] * 4),                              # an odd number of paired blocks in phase 0 ...
            ([above, 40] + pairable[-5:], [NODEP, NODEP] + [0] * 5)]           # ... and in phase 1
    wide = [k for k in LEGAL_K if k <= kmax and h.lsnh_turbo_nwin(k) > 64]
    if wide:
        sets.append(([max(wide), below, max(wide), 40], [NODEP, NODEP, 0, 0]))
    for trial in range(40):
        n = int(rng.integers(0, 401))
        pool = LEGAL_K if trial % 3 else [int(k) for k in rng.choice(LEGAL_K, 5)]      # (few sizes: many equal K)
        K = [int(k) for k in rng.choice(pool, n)]
        dep = [NODEP if (i == 0 or rng.random() < (0.0, 0.3, 1.0)[trial % 3]) else int(rng.integers(0, i)) for i in range(n)]
        sets.append((K, dep))
    return sets, wide


def test_turbo_packed_order_against_a_stable_sort():
    """turbo_packed_order (the order in which k_turbo sees the blocks of a downlink launch) against the key written out here and sorted by Python's stable sort:
    phase (blocks that depend on nothing first), solo before paired, K descending, index ascending; paired = K <= LSN_TURBO_PAIR_KMAX and at most 64 trellis
    windows.  Order, the four counts and both maxima.  The second condition of `paired` never decides: every legal K up to LSN_TURBO_PAIR_KMAX has at most 64
    windows (asserted below), so no set can hold a block that it alone keeps solo."""
    h = hosttest()
    kmax = h.lsnh_turbo_pair_kmax()
    assert len(LEGAL_K) == 188 and kmax in LEGAL_K
    sets, wide = _packed_order_sets()
    assert wide == []
    odd = 0
    for K, dep in sets:
        n = len(K)
        pair = [k <= kmax and h.lsnh_turbo_nwin(k) <= 64 for k in K]
        phase = [0 if d == NODEP else 1 for d in dep]
        want = sorted(range(n), key=lambda i: (phase[i], pair[i], -K[i]))
        counts = [sum(1 for i in range(n) if phase[i] == ph and pair[i] == pr) for pr in (False, True) for ph in (0, 1)]
        maxima = [max([K[i] for i in range(n) if pair[i] == pr], default=0) for pr in (False, True)]
        odd += counts[2] % 2 + counts[3] % 2
        Ka, da = np.array(K, dtype=np.uint32), np.array(dep, dtype=np.uint32)
        order, out6 = np.full(n, 0xFFFFFFFF, dtype=np.uint32), np.zeros(6, dtype=np.uint32)
        h.lsnh_turbo_packed_order(n, Ka.ctypes.data, da.ctypes.data, order.ctypes.data, out6.ctypes.data)
        assert list(order) == want, (K, dep)
        assert list(out6) == counts + maxima, (K, dep)
    assert odd


def test_turbo_place_lays_the_blocks_out_in_launch_order():
    """turbo_place (the soft-data layout of runJobs and puschDecodeGrid): offsets are multiples of 4, ascend in launch order from the base and do not overlap
    (K + 12 words each), spp_n = sum of LSN_SPP_WORDS(K), the inverse map inverts the order, emax is the largest E, and launch position i holds block order[i]."""
    h = hosttest()
    rng = np.random.default_rng(12)
    for si, (K, dep) in enumerate(_packed_order_sets()[0]):
        n = len(K)
        Ka, da, E = np.array(K, dtype=np.uint32), np.array(dep, dtype=np.uint32), rng.integers(1, 40000, n).astype(np.uint32)
        order, out6 = np.zeros(n, dtype=np.uint32), np.zeros(6, dtype=np.uint32)
        h.lsnh_turbo_packed_order(n, Ka.ctypes.data, da.ctypes.data, order.ctypes.data, out6.ctypes.data)
        base = 0 if si % 2 else 4 * int(rng.integers(0, 1000))
        placed, spp_of, out2 = np.zeros((n, 4), dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(2, dtype=np.uint64)
        h.lsnh_turbo_place(n, Ka.ctypes.data, E.ctypes.data, order.ctypes.data, base, placed.ctypes.data, spp_of.ctypes.data, out2.ctypes.data)
        words = [h.lsnh_spp_words(k) for k in K]
        assert all(w % 4 == 0 and k + 12 <= w < k + 16 for w, k in zip(words, K))
        assert int(out2[0]) == sum(words) and int(out2[1]) == (int(E.max()) if n else 0)
        at = base
        for i in range(n):
            q = int(order[i])
            assert list(placed[i]) == [K[q], int(E[q]), at, q] and at % 4 == 0 and int(spp_of[q]) == at
            at += words[q]
        assert at == base + int(out2[0])


def test_turbo_order_and_placement_under_sanitizers():
    """the same two functions in a program of its own built with -fsanitize=address,undefined (the counting sort indexes a table by K)"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "_build/test_turbo_order"], stdout=subprocess.DEVNULL)
    out = subprocess.check_output([os.path.join(ROOT, "tests", "native", "_build", "test_turbo_order")]).decode()
    assert out.startswith("OK")


def test_commit_walk_under_sanitizers():
    """the commit walk (csrc/host/lsn_commit.h) with a scripted decoder in a program of its own built with -fsanitize=address,undefined: random DCIs through
    finishSubframe, the commit view and the walk, tracking database off / on / both tables, HARQ on"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "_build/test_commit_walk"], stdout=subprocess.DEVNULL)
    out = subprocess.check_output([os.path.join(ROOT, "tests", "native", "_build", "test_commit_walk")]).decode()
    assert out.startswith("OK")


def _search_parity(scn, nsf, seed, update_meta_period=0, **over):
    """FALCON search of the product over oracle-decoded candidate tables == the oracle worker's own search."""
    h = hosttest()
    sc = scenario(scn, seed=seed, **over)
    tx = TxGen(**sc)
    ow = OracleWorker(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], sc["nof_rx"], sc["phich_ng_x6"])
    regs_cce = None
    hs = None
    total = 0
    for i in range(nsf):
        tti, iq, pdus = tx.next()
        upd = 1 if (update_meta_period and i % update_meta_period == 0) else 0
        ow.work(iq, tti, update_meta=upd)
        if hs is None:
            # nof_cce per CFI from the oracle's REG tables
            from lsn_testlib import oracle as _o

            class Regs(C.Structure):
                _fields_ = [("nof_regs", C.c_uint32 * 3), ("nof_cce", C.c_uint32 * 3), ("k0", (C.c_uint16 * 800) * 3),
                            ("l", (C.c_uint8 * 800) * 3), ("pcfich_k0", C.c_uint16 * 4), ("ngroups_phich", C.c_uint32)]
            regs = Regs()
            cell = OCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], sc["phich_ng_x6"])
            _o().o_regs_init.argtypes = [C.POINTER(OCell), C.c_void_p]
            _o().o_regs_init(C.byref(cell), C.byref(regs))
            regs_cce = (C.c_uint32 * 3)(*regs.nof_cce)
            hs = h.lsnh_search_new(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], regs_cce, 5, 0.99, 0)
            sizes = [h.lsnh_search_size(hs, k) for k in range(h.lsnh_search_nof_sizes(hs))]
        cfi = ow.cfi()
        cand, pw = candidate_table(ow.llr(), regs_cce[cfi - 1], sizes, tti % 10)
        out = (C.c_uint32 * (64 * 6))()
        n = h.lsnh_search_run(hs, tti, cfi, float(ow.chest().snr_db), cand, pw.ctypes.data, upd, out, 64 * 6)
        got = [tuple(out[6 * k:6 * k + 6]) for k in range(n)]
        exp = ow.accepted()
        assert got == exp, (i, got, exp)
        # RAR feedback (decode results are the oracle's here): keep the RNTI managers in step
        total += n
        assert h.lsnh_search_nof_active(hs) <= ow.nof_active() + 64
    st = (C.c_uint32 * 7)()
    h.lsnh_search_stats(hs, st)
    os_ = ow.stats()
    assert list(st) == [os_.nof_decoded_locations, os_.nof_cce, os_.nof_missed_cce, os_.nof_subframes,
                        os_.nof_subframe_collisions_dw, os_.nof_subframe_collisions_up, os_.nof_locations]
    h.lsnh_search_free(hs)
    assert total > 0
    return total


def test_falcon_search_small_cell():
    _search_parity("small", 30, seed=4)


def test_falcon_search_cfg1():
    _search_parity("cfg1", 25, seed=1)


def test_falcon_search_15mhz_cell():
    _search_parity("cfg2", 12, seed=6, nof_prb=75, cell_id=77, n_rnti=20)


def test_falcon_search_four_port_cells():
    """the product's host search on four-port candidate tables (four-port DCI sizes of formats 2 / 2A, 76 CCEs at 20 MHz) == the oracle worker's"""
    _search_parity("cfg2", 14, seed=7, nof_ports=4, cfi=0, n_rnti=12)
    _search_parity("cfg3", 12, seed=8, nof_ports=4, nof_prb=50, n_rnti=20, rar_period=0)


def test_falcon_search_cfg3_meta_update():
    _search_parity("cfg3", 16, seed=3, update_meta_period=8, rar_period=0)


# ---- ingest: the staging ring and the sample-format rule (lsn_types.h)
def _ring_api():
    h = hosttest()
    h.lsnh_ring_new.restype = C.c_void_p
    h.lsnh_ring_new.argtypes = [C.c_uint32]
    h.lsnh_ring_free.argtypes = [C.c_void_p]
    h.lsnh_ring_slots.restype = C.c_uint32
    h.lsnh_ring_slots.argtypes = [C.c_void_p]
    h.lsnh_ring_acquire.restype = C.c_uint32
    h.lsnh_ring_acquire.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    h.lsnh_ring_retire.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    return h


@pytest.mark.parametrize("nslots", [3, 12])
def test_staging_ring_hands_every_user_the_mark_of_the_slots_last_retire(nslots):
    """A seeded script of acquire / retire calls by several "paths" (worker pool, process_host, peer copy: the ring cannot tell them apart) with increasing
    marks.  Slots come round-robin; a slot nobody has retired asks for no wait (0); otherwise acquire returns exactly the mark of the slot's last retire,
    whoever recorded it - what lsn_phy_put_pending followed by lsn_phy_process_host without a join in between depends on."""
    h = _ring_api()
    ring = h.lsnh_ring_new(nslots)
    try:
        assert h.lsnh_ring_slots(ring) == nslots
        rng = np.random.default_rng(100 + nslots)
        last = {}                      # slot -> (mark, path) of its last retire: the model
        held = []                      # acquired, not retired yet: (slot, path)
        mark, count, waited_for_other = 0, 0, 0
        for _ in range(40 * nslots):
            if held and (len(held) >= 3 or rng.random() < 0.5):   # retire one of the blocks in flight, not always the oldest
                slot, path = held.pop(int(rng.integers(len(held))))
                mark += int(rng.integers(1, 5))                   # a submit of one to four chunks
                h.lsnh_ring_retire(ring, slot, mark)
                last[slot] = (mark, path)
            else:
                w = C.c_uint64(0xDEAD)
                slot = h.lsnh_ring_acquire(ring, C.byref(w))
                path = int(rng.integers(3))
                assert slot == count % nslots
                assert w.value == (last[slot][0] if slot in last else 0)
                if slot in last and last[slot][1] != path:
                    waited_for_other += 1
                held.append((slot, path))
                count += 1
        assert count > 3 * nslots and waited_for_other > nslots   # the ring wrapped, and paths met each other's marks
    finally:
        h.lsnh_ring_free(ring)


FMT_BYTES = {0: 8, 1: 4, 2: 2}                                 # LSN_FILE_CF32 / SC16 / SC8: bytes of one complex sample
FMT_DEFAULT = {1: 1.0 / 32768.0, 2: 1.0 / 128.0}               # scale 0 = full scale -> 1.0
FMT_SCALES = [0.0, 2.0 ** -11, 3e-5, float("nan"), float("inf"), -1.0]


def _format_table():
    """(format, scale) -> (valid, bytes, effective scale), written out: cf32 is taken as it is, whatever its scale field holds; integer samples want a finite
    scale >= 0 and 0 selects the default; formats above SC8 do not exist"""
    t = {}
    for s in FMT_SCALES:
        t[(0, s)] = (True, 8, 1.0)
        for f in (1, 2):
            ok = s in (0.0, 2.0 ** -11, 3e-5)
            t[(f, s)] = (ok, FMT_BYTES[f], np.float32(s if s else FMT_DEFAULT[f])) if ok else (False, None, None)
        t[(3, s)] = (False, None, None)
    t[(0xFFFFFFFF, 0.0)] = (False, None, None)
    return t


def test_sample_format_rule_against_the_written_table():
    h = hosttest()
    h.lsnh_sample_format.argtypes = [C.c_uint32, C.c_float, C.c_void_p]
    tab = _format_table()
    assert len(tab) == 4 * 6 + 1
    for (fmt, scale), (ok, nbytes, eff) in tab.items():
        out = (C.c_float * 3)()
        h.lsnh_sample_format(fmt, scale, out)
        assert bool(out[0]) == ok, (fmt, scale)
        if ok:
            assert int(out[1]) == nbytes and np.float32(out[2]) == np.float32(eff), (fmt, scale, out[1], out[2])


def test_sample_format_rule_through_lsn_resample_span():
    """the same verdicts where the rule is reachable without a device: lsn_resample_span refuses (LSN_ERROR_INVALID_INPUTS, -2) exactly the rows the table calls invalid"""
    import ltesniffer_amd as la
    for (fmt, scale), (ok, _, _) in _format_table().items():
        cfg = la._resample_cfg(1, 23.04e6, 30.72e6, 0, 0.0, 0, 0, 0.0, fmt, scale)
        sp = la.ResampleSpan()
        r = la.lib().lsn_resample_span(C.byref(cfg), 1000, 100000, C.byref(sp))
        assert r == (0 if ok else -2), (fmt, scale, r)

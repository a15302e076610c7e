"""A PUSCH transmitter written from TS 36.211 / 36.212 / 36.213 alone, in float64 numpy (test infrastructure only).

Transport block -> CRC24A -> segmentation -> turbo encoder -> rate matching (N_L = 1) -> concatenation (36.212 5.2.2.1 - 5.2.2.5), data / control
multiplexing (5.2.2.7), channel interleaver (5.2.2.8, the standard's procedure run literally on a matrix of cells), scrambling (36.211 5.3.1),
modulation (5.3.2), transform precoding (5.3.3), mapping (5.3.4), demodulation reference signal (5.5.1, 5.5.2.1), SC-FDMA baseband (5.6, synthesised
directly from the formula), through a per-grant complex gain, an optional integer delay inside the cyclic prefix and optional AWGN.  It follows no
line of the synthetic transmitter (tools/txgen), the oracle (oracle/o_pusch.c) or the product (lsn_ul.cc, stage_ul.hip), and reuses only spec-derived
test code: CRC, segmentation, turbo encoder, rate matching, block sizes E and the four constellations of tests/spec_pdsch.py, the Gold generator of
tests/second_frontend.py and the type-1 hopping offset of tests/lsn_testlib.py (pusch_hop_slot1).

The control information is NOT encoded.  The receiver under test locates HARQ-ACK, RI and CQI cells and never decodes them, so the control cells
carry random bits mapped on the grant's constellation: only their NUMBER (Q' of 5.2.2.6 with its caps) and their PLACE (5.2.2.7, 5.2.2.8) follow the
specification.  (The placeholder bits x / y that 36.211 5.3.1 treats specially only occur inside encoded HARQ-ACK / RI words: with random control
bits every bit is scrambled alike.)

Shared on purpose, hence COMMON-MODE and not covered by the tests built on this file:
  * the base sequences phi(n) for one and two PRB (36.211 Tables 5.5.1.2-1 / -2) are read from spec/lte_tables.h with the regex reader of
    tests/test_spec_tables.py: there is no second copy of them to compare with (the product counts decodes that relied on them,
    lsn_perf_t.nof_pusch_on_unverified_dmrs);
  * the transport block sizes (36.213 Table 7.1.7.2.1-1), as in tests/spec_pdsch.py;
  * the QPP interleaver parameters, through tests/spec_pdsch.py.
NOT shared, written out below: the beta offsets of 36.213 Tables 8.6.3-1 / -2 / -3, both n_DMRS tables, the column sets of 36.212 Tables
5.2.2.8-1 / -2, the uplink MCS map of 36.213 Table 8.6.1-1.

Assumptions: an initial transmission in the same subframe (M_sc^PUSCH-initial = M_sc^PUSCH, N_symb^PUSCH-initial = N_symb^PUSCH), no SRS, one layer,
N_cb = K_w."""
from fractions import Fraction

import numpy as np

import second_frontend as S
import spec_pdsch as SP
from test_spec_tables import _rows

FFT = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}
# 36.213 Table 8.6.3-1 (HARQ-ACK, index 0..14), -2 (RI, 0..12), -3 (CQI, 2..15); every other index is reserved
BETA_ACK = (2, 2.5, 3.125, 4, 5, 6.25, 8, 10, 12.625, 15.875, 20, 31, 50, 80, 126)
BETA_RI = (1.25, 1.625, 2, 2.5, 3.125, 4, 5, 6.25, 8, 10, 12.625, 15.875, 20)
BETA_CQI = (None, None, 1.125, 1.25, 1.375, 1.625, 1.75, 2, 2.25, 2.5, 2.875, 3.125, 3.5, 4, 5, 6.25)
DEFAULT_BETA_IDX = dict(ack=10, cqi=8, ri=11)    # what the receiver assumes until it has seen an RRC set-up (beta = 20, 2.25, 15.875)
# 36.211 Table 5.5.2.1.1-2: cyclicShift of SIB2 -> n_DMRS^(1); Table 5.5.2.1.1-1: cyclic shift field of DCI format 0 -> n_DMRS^(2)
N_DMRS1 = (0, 2, 3, 4, 6, 8, 9, 10)
N_DMRS2 = (0, 6, 3, 4, 2, 8, 10, 9)
# 36.212 Tables 5.2.2.8-1 (rank indication) and 5.2.2.8-2 (HARQ-ACK): the column sets, normal / extended cyclic prefix
COLS_RI = {0: (1, 4, 7, 10), 1: (0, 3, 5, 8)}
COLS_ACK = {0: (2, 3, 8, 9), 1: (1, 2, 6, 7)}
# 36.213 Table 8.6.1-1: MCS 0..10 QPSK I_TBS = MCS, 11..20 16QAM I_TBS = MCS - 1, 21..28 64QAM I_TBS = MCS - 2
MCS_UL = {m: (2, m) for m in range(11)}
MCS_UL.update({m: (4, m - 1) for m in range(11, 21)})
MCS_UL.update({m: (6, m - 2) for m in range(21, 29)})
PHI = {12: _rows("lsn_dmrs_phi12"), 24: _rows("lsn_dmrs_phi24")}    # COMMON-MODE (docstring)
assert all(len(PHI[m]) == 30 and all(len(r) == m and set(r) <= {-3, -1, 1, 3} for r in PHI[m]) for m in (12, 24))

CQI, RI, ACK, DATA = 1, 2, 3, 0


def tbs_of(mcs, L, qm=None):
    """36.213 8.6.1 / 8.6.2: -> (Q_m, TBS) of an uplink MCS index on L PRB; qm overrides the modulation (a 256QAM transmission with the same block size)"""
    q, itbs = MCS_UL[mcs]
    return (qm or q), SP._TBS_FILE[itbs][L - 1]


# ---------------------------------------------------------------------------------------------------------------------------- control information (36.212 5.2.2.6)
def n_symb_pusch(cp):
    """N_symb^PUSCH = 2 (N_symb^UL - 1) - N_SRS: 12 with the normal cyclic prefix, 10 with the extended one (no SRS)"""
    return 2 * ((6 if cp else 7) - 1)


def q_prime(O, M_sc, nsymb, beta, sum_K, cap):
    """5.2.2.6: Q' = min(ceil(O M_sc^initial N_symb^initial beta / sum_r K_r), cap), in exact arithmetic (every beta is a multiple of 1/8)"""
    if O <= 0:
        return 0
    v = Fraction(O * M_sc * nsymb) * Fraction(beta) / sum_K
    return min(-((-v.numerator) // v.denominator), cap)


def uci_sizes(M_sc, cp, sum_K, nof_ack=0, ri_bits=0, cqi_bits=0, i_ack=None, i_ri=None, i_cqi=None):
    """-> (Q'_ACK, Q'_RI, Q'_CQI) in modulation symbols.  Caps: 4 M_sc for HARQ-ACK and RI; M_sc N_symb - Q'_RI (= Q_RI / Q_m) for the CQI, whose O
    counts L = 8 CRC bits more when O > 11"""
    ns = n_symb_pusch(cp)
    ia, ir, ic = (DEFAULT_BETA_IDX["ack"] if i_ack is None else i_ack, DEFAULT_BETA_IDX["ri"] if i_ri is None else i_ri,
                  DEFAULT_BETA_IDX["cqi"] if i_cqi is None else i_cqi)
    qa = q_prime(nof_ack, M_sc, ns, BETA_ACK[ia], sum_K, 4 * M_sc)
    qr = q_prime(ri_bits, M_sc, ns, BETA_RI[ir], sum_K, 4 * M_sc)
    qc = q_prime(cqi_bits + (8 if cqi_bits > 11 else 0), M_sc, ns, BETA_CQI[ic], sum_K, M_sc * ns - qr) if cqi_bits else 0
    return qa, qr, qc


# ---------------------------------------------------------------------------------------------------------------------------- multiplexing and interleaver (5.2.2.7, 5.2.2.8)
def interleave(M_sc, cp, q_ack, q_ri, q_cqi):
    """The procedure of 5.2.2.8 on a matrix of cells (one cell = one vector of Q_m bits = one modulation symbol), R'_mux = M_sc rows, C_mux = N_symb^PUSCH
    columns.  (1) the rank-indication vectors go into the columns of Table 5.2.2.8-1, from the last row upwards (i counts vectors, r = R' - 1 -
    floor(i / 4), the column index j advances by 3 modulo 4); (2) the vectors g_0 .. g_H'-1 of 5.2.2.7 - Q'_CQI control vectors first, the UL-SCH
    vectors behind - are written row by row into the cells that are still free; (3) the HARQ-ACK vectors overwrite, same walk, Table 5.2.2.8-2;
    (4) the matrix is read column by column.
    -> (kind[n], gidx[n]) in transmitted order, n = M_sc C_mux: the kind of each cell and, for CQI / DATA / ACK cells, the index k of the vector g_k that
    was written there first (for an ACK cell: the vector it overwrote)"""
    C = n_symb_pusch(cp)
    R = M_sc
    kind = [[None] * C for _ in range(R)]
    g = [[-1] * C for _ in range(R)]
    i, j, r = 0, 0, R - 1
    while i < q_ri:
        kind[r][COLS_RI[cp][j]] = RI
        i += 1
        r = R - 1 - i // 4
        j = (j + 3) % 4
    k = 0
    for r in range(R):
        for c in range(C):
            if kind[r][c] is None:
                kind[r][c] = CQI if k < q_cqi else DATA
                g[r][c] = k
                k += 1
    assert k == R * C - q_ri
    i, j, r = 0, 0, R - 1
    while i < q_ack:
        kind[r][COLS_ACK[cp][j]] = ACK
        i += 1
        r = R - 1 - i // 4
        j = (j + 3) % 4
    order = [(r, c) for c in range(C) for r in range(R)]
    return np.array([kind[r][c] for r, c in order]), np.array([g[r][c] for r, c in order])


# ---------------------------------------------------------------------------------------------------------------------------- reference signal (36.211 5.5.1, 5.5.2.1)
def f_ss_pusch(cell_id, delta_ss):
    """5.5.1.3: f_ss^PUCCH = N_ID mod 30, f_ss^PUSCH = (f_ss^PUCCH + Delta_ss) mod 30"""
    return (cell_id % 30 + delta_ss) % 30


def group_and_sequence(cell_id, delta_ss, group_hopping, sequence_hopping, ns, M_sc):
    """5.5.1.3 / 5.5.1.4 -> (u, v) of slot ns.  f_gh = (sum_i c(8 ns + i) 2^i) mod 30 with c_init = floor(N_ID / 30) when group hopping is on; v = c(ns)
    with c_init = floor(N_ID / 30) 2^5 + f_ss^PUSCH when sequence hopping is on, group hopping off and M_sc >= 6 N_sc^RB"""
    fss = f_ss_pusch(cell_id, delta_ss)
    fgh = 0
    if group_hopping:
        c = S.gold(cell_id // 30, 8 * 20)
        fgh = sum(int(c[8 * ns + i]) << i for i in range(8)) % 30
    v = 0
    if sequence_hopping and not group_hopping and M_sc >= 72:
        v = int(S.gold((cell_id // 30) * 32 + fss, 20)[ns])
    return (fgh + fss) % 30, v


def base_sequence(u, v, M_sc):
    """5.5.1.1: x_q(n mod N_ZC), x_q(m) = exp(-j pi q m (m + 1) / N_ZC), q = floor(qbar + 1/2) + v (-1)^floor(2 qbar), qbar = N_ZC (u + 1) / 31, N_ZC the
    largest prime below M_sc; 5.5.1.2: exp(j phi(n) pi / 4) for one and two PRB"""
    if M_sc in PHI:
        return np.exp(1j * np.pi * np.array(PHI[M_sc][u], dtype=np.float64) / 4)
    assert M_sc >= 36
    nzc = max(p for p in range(2, M_sc) if all(p % d for d in range(2, p)))
    qbar = Fraction(nzc * (u + 1), 31)
    q = int((qbar + Fraction(1, 2)) // 1) + v * (-1) ** int((2 * qbar) // 1)
    m = np.arange(M_sc) % nzc
    return np.exp(-1j * np.pi * ((q * m * (m + 1)) % (2 * nzc)) / nzc)


def n_cs(cell_id, delta_ss, cyclic_shift, dci_field, ns, cp):
    """5.5.2.1.1: n_cs = (n_DMRS^(1) + n_DMRS^(2) + n_PN(ns)) mod 12, n_PN = sum_i c(8 N_symb^UL ns + i) 2^i, c_init = floor(N_ID / 30) 2^5 + f_ss^PUSCH"""
    nsl = 6 if cp else 7
    c = S.gold((cell_id // 30) * 32 + f_ss_pusch(cell_id, delta_ss), 8 * nsl * 20 + 8)
    npn = sum(int(c[8 * nsl * ns + i]) << i for i in range(8))
    return (N_DMRS1[cyclic_shift] + N_DMRS2[dci_field] + npn) % 12


def dmrs(cell, ns, dci_field, M_sc):
    """r_PUSCH of slot ns: exp(j alpha n) rbar_u,v(n), alpha = 2 pi n_cs / 12"""
    u, v = group_and_sequence(cell["cell_id"], cell["delta_ss"], cell["group_hopping"], cell["sequence_hopping"], ns, M_sc)
    a = 2 * np.pi * n_cs(cell["cell_id"], cell["delta_ss"], cell["cyclic_shift"], dci_field, ns, cell["cp"]) / 12
    return np.exp(1j * a * np.arange(M_sc)) * base_sequence(u, v, M_sc)


# ---------------------------------------------------------------------------------------------------------------------------- one grant -> resource grid
def transform_precode(d, M_sc):
    """5.3.3: z(l M_sc + k) = 1 / sqrt(M_sc) sum_i d(l M_sc + i) exp(-j 2 pi i k / M_sc), written as the matrix it is"""
    i = np.arange(M_sc)
    W = np.exp(-2j * np.pi * np.outer(i, i) / M_sc) / np.sqrt(M_sc)
    return (np.asarray(d).reshape(-1, M_sc) @ W.T).reshape(-1)


def build_grant(cell, sf_idx, g, rng):
    """g: dict(rnti, n_prb, L_prb, mod, tbs, rv, n_dmrs: the DCI field; optional n_prb2 (slot 1, type-1 hopping), nof_ack, ri_bits, cqi_bits,
    i_ack / i_ri / i_cqi: beta indices, bits: the payload).  -> (a[nsym, 12 nof_prb]: its resource elements, truth dict)"""
    cp, nre = cell["cp"], 12 * cell["nof_prb"]
    nsl = 6 if cp else 7
    M, Qm, C = 12 * g["L_prb"], g["mod"], n_symb_pusch(cp)
    bits = np.asarray(g["bits"] if "bits" in g else rng.integers(0, 2, g["tbs"]), dtype=np.uint8)
    assert len(bits) == g["tbs"]
    cbs, seg = SP.code_blocks(bits)
    qa, qr, qc = uci_sizes(M, cp, sum(seg["Ks"]), g.get("nof_ack", 0), g.get("ri_bits", 0), g.get("cqi_bits", 0), g.get("i_ack"), g.get("i_ri"), g.get("i_cqi"))
    G = Qm * (M * C - qr - qc)
    assert G > 0
    Es = SP.block_sizes_E(G, seg["C"], 1, Qm)
    blocks, f = [], []
    for r, c in enumerate(cbs):
        d = SP.turbo_encode(c)
        e, src = SP.rate_match(d, Es[r], g["rv"])
        blocks.append(dict(K=len(c), F=seg["F"] if r == 0 else 0, E=Es[r], d=d, src=src))
        f.append(e)
    f = np.concatenate(f)
    assert len(f) == G
    kind, gidx = interleave(M, cp, qa, qr, qc)
    # the bits of every cell in transmitted order: UL-SCH vectors from f, every control vector random (module docstring)
    h = rng.integers(0, 2, (M * C, Qm)).astype(np.uint8)
    data = kind == DATA
    h[data] = f.reshape(-1, Qm)[gidx[data] - qc]
    over = (kind == ACK) & (gidx >= qc)             # HARQ-ACK vectors that overwrote UL-SCH vectors
    punct = np.zeros(G, dtype=bool)
    punct.reshape(-1, Qm)[gidx[over] - qc] = True
    assert np.sum(kind == ACK) == qa and np.sum(kind == RI) == qr and np.sum(data) + np.sum(over) == G // Qm
    # 36.211 5.3.1: c_init = n_RNTI 2^14 + floor(ns / 2) 2^9 + N_ID, over the transmitted order
    c = S.gold(g["rnti"] * 2 ** 14 + sf_idx * 2 ** 9 + cell["cell_id"], M * C * Qm)
    z = transform_precode(SP.modulate(h.reshape(-1) ^ c, Qm), M).reshape(C, M)
    a = np.zeros((2 * nsl, nre), dtype=np.complex128)
    k0 = (12 * g["n_prb"], 12 * g.get("n_prb2", g["n_prb"]))
    rs = nsl - 4     # 5.5.2.1.2: l = 3 (normal) / l = 2 (extended) of each slot
    col = 0
    for l in range(2 * nsl):
        slot = l // nsl
        if l % nsl == rs:
            a[l, k0[slot]:k0[slot] + M] = dmrs(cell, 2 * sf_idx + slot, g["n_dmrs"], M)
        else:
            a[l, k0[slot]:k0[slot] + M] = z[col]   # 5.3.4: k first, then l, the reference-signal symbols skipped
            col += 1
    assert col == C
    return a, dict(payload=np.packbits(bits).tobytes(), bits=bits, seg=seg, blocks=blocks, rv=g["rv"], f=f, G=G, punct=punct, q_ack=qa, q_ri=qr, q_cqi=qc,
                   Qm=Qm, kind=kind, gidx=gidx, grant=dict(g))


# ---------------------------------------------------------------------------------------------------------------------------- SC-FDMA baseband (36.211 5.6)
def scfdma(a, nof_prb, cp):
    """s_l(t) = sum_k a_k(-),l exp(j 2 pi (k + 1/2) Delta_f (t - N_CP,l T_s)), k = -floor(N_RB N_sc / 2) .. ceil(N_RB N_sc / 2) - 1, k(-) = k + floor(N_RB N_sc / 2),
    0 <= t < (N_CP,l + N) T_s, sampled at t = n T_s with 1 / T_s = N Delta_f; the symbols one after the other (Table 5.6-1: N_CP = 160 / 144 of 2048, or
    512 with the extended cyclic prefix).  No carrier is left out at DC.  Scaled by 1 / N, so that an N-point DFT returns a.  -> x[15 N] complex128"""
    N, nre = FFT[nof_prb], 12 * nof_prb
    nsl = a.shape[0] // 2
    kk = np.nonzero(np.any(a != 0, axis=0))[0]
    x = np.zeros(15 * N, dtype=np.complex128)
    pos = 0
    basis = {}
    for l in range(a.shape[0]):
        ncp = (512 if cp else 160 if l % nsl == 0 else 144) * N // 2048
        if ncp not in basis:
            n = np.arange(ncp + N) - ncp
            basis[ncp] = np.exp(2j * np.pi * np.outer(n, kk - nre // 2 + 0.5) / N)
        x[pos:pos + ncp + N] = basis[ncp] @ a[l, kk] / N
        pos += ncp + N
    assert pos == 15 * N
    return x


def ideal_demod(x, nof_prb, cp):
    """the inverse of scfdma in float64, by correlation with the same exponentials over the useful part of each symbol -> a[nsym, 12 nof_prb]"""
    N, nre = FFT[nof_prb], 12 * nof_prb
    nsl = 6 if cp else 7
    n = np.arange(N)
    B = np.exp(-2j * np.pi * np.outer(np.arange(nre) - nre // 2 + 0.5, n) / N)
    a = np.zeros((2 * nsl, nre), dtype=np.complex128)
    pos = 0
    for l in range(2 * nsl):
        pos += (512 if cp else 160 if l % nsl == 0 else 144) * N // 2048
        a[l] = B @ x[pos:pos + N]
        pos += N
    return a


def subframe(cell, sf_idx, grants, seed=0, snr_db=None):
    """cell: dict(nof_prb, cell_id, cp, cyclic_shift, delta_ss, group_hopping, sequence_hopping).  grants: build_grant dicts, plus per grant gain_db,
    phase (default: random, +-3 dB), delay: whole samples, inside the cyclic prefix.  The grants add up.  AWGN: variance 10^(-snr_db / 10) per resource
    element, against a grant of unit gain, from its own generator so that the signal does not depend on it.
    -> (iq[15 N] complex64, [truth per grant])"""
    rng = np.random.default_rng(seed)
    N = FFT[cell["nof_prb"]]
    x = np.zeros(15 * N, dtype=np.complex128)
    truths = []
    used = np.zeros((2, cell["nof_prb"]), dtype=bool)
    for g in grants:
        a, t = build_grant(cell, sf_idx, g, rng)
        for s, n in enumerate((g["n_prb"], g.get("n_prb2", g["n_prb"]))):
            assert n + g["L_prb"] <= cell["nof_prb"] and not used[s, n:n + g["L_prb"]].any(), "grants overlap"
            used[s, n:n + g["L_prb"]] = True
        gain = 10 ** (g.get("gain_db", rng.uniform(-3, 3)) / 20) * np.exp(1j * g.get("phase", rng.uniform(0, 2 * np.pi)))
        d = g.get("delay", 0)
        assert 0 <= d < 144 * N // 2048
        y = gain * scfdma(a, cell["nof_prb"], cell["cp"])
        x += np.concatenate([np.zeros(d), y[:len(y) - d]])
        t.update(gain=gain, delay=d)
        truths.append(t)
    if snr_db is not None:
        nr = np.random.default_rng(100000 + seed)
        sd = np.sqrt(10 ** (-snr_db / 10) / N / 2)     # the receiver's unnormalised N-point DFT multiplies the per-sample variance by N
        x = x + sd * (nr.standard_normal(len(x)) + 1j * nr.standard_normal(len(x)))
    return x.astype(np.complex64), truths


def hop_slot1_spec(nof_prb, hop_offset, hop_bits, rb_start):
    """36.213 8.4.1 to the letter, type 1: n_PRB^S1 = RB_START = ntilde^S1 + Ntilde_HO / 2; ntilde of slot 1 from Table 8.4-2 on ntilde^S1; n_PRB of slot 1 =
    ntilde + Ntilde_HO / 2 (Ntilde_HO = N_HO rounded up to even; N_RB^PUSCH = N_RB^UL - Ntilde_HO - (N_RB^UL mod 2)).  None for type 2.  See
    tests/test_spec_pusch_oracle.py::test_type1_hopping_offset_against_the_letter_of_the_specification for where the receiver's rule differs"""
    ho = hop_offset + hop_offset % 2
    n = nof_prb - ho - nof_prb % 2
    kind = {0: "half", 1: None}[hop_bits] if nof_prb < 50 else {0: "quart", 1: "quart_neg", 2: "half", 3: None}[hop_bits]
    if kind is None:
        return None
    t = rb_start - ho // 2
    nt = {"quart": (n // 4 + t) % n, "quart_neg": (t - n // 4) % n, "half": (n // 2 + t) % n}[kind]
    return nt + ho // 2

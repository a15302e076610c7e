"""A PDSCH transmit chain written from TS 36.211 / 36.212 / 36.213 alone, in float64 numpy (test infrastructure only).

Transport block -> CRC24A -> code-block segmentation -> turbo encoder -> rate matching -> concatenation (36.212 5.1.1 - 5.1.5, 5.3.2), scrambling ->
modulation -> layer mapping -> precoding -> resource elements (36.211 6.3.1 - 6.3.5).  It shares no line and no table with the synthetic transmitter
(tools/txgen), the oracle (oracle/) or the product, and reuses only spec-derived test code: the Gold generator and the CRS of tests/second_frontend.py
and the transmit-diversity precoder of tests/spec_downlink.py.

Shared on purpose, hence COMMON-MODE and not covered by the tests built on this file:
  * the QPP interleaver parameters f1, f2 (36.212 Table 5.1.3-3) and the transport block sizes (36.213 Table 7.1.7.2.1-1) are read from
    spec/lte_tables.h with the regex reader of tests/test_spec_tables.py - there is no other copy of those tables to compare with, and that test pins
    part of them.  (The 188 block sizes K themselves are generated below from the step rule of the table and compared with the file.)
  * the MCS -> (Q_m, I_TBS) map of the 256QAM table (36.213 Table 7.1.7.1-1A) is read from the same file.
The 64QAM-table map (Table 7.1.7.1-1) is NOT shared: it is written out below.

Assumption: N_cb = K_w, i.e. no soft-buffer limit (36.212 5.1.4.1.2 with N_IR large: UE category and K_MIMO are unknown to a sniffer), which is what the
receiver assumes too.  Power: rho_A = rho_B = 1 (P_A = 0 dB; P_B = 0 on one port, 1 on two or four ports, 36.213 Table 5.2-1), so every PDSCH
resource element has the energy of a CRS element."""
import re

import numpy as np

import second_frontend as S
import spec_downlink as SD
from test_spec_tables import QPP as _QPP_FILE, SRC as _TABLES_SRC, TBS as _TBS_FILE

# ---------------------------------------------------------------------------------------------------------------------------- tables
# 36.212 Table 5.1.3-3: the block sizes follow a step rule (40..512 by 8, ..1024 by 16, ..2048 by 32, ..6144 by 64); f1, f2 are common-mode (docstring)
K_SIZES = list(range(40, 512, 8)) + list(range(512, 1024, 16)) + list(range(1024, 2048, 32)) + list(range(2048, 6144 + 1, 64))
QPP_F = {k: (f1, f2) for k, f1, f2 in _QPP_FILE}
assert sorted(QPP_F) == K_SIZES and len(K_SIZES) == 188
# 36.213 Table 7.1.7.1-1, written out: MCS 0..9 QPSK I_TBS = MCS, 10..16 16QAM I_TBS = MCS - 1, 17..28 64QAM I_TBS = MCS - 2
MCS_64QAM = {m: (2, m) for m in range(10)}
MCS_64QAM.update({m: (4, m - 1) for m in range(10, 17)})
MCS_64QAM.update({m: (6, m - 2) for m in range(17, 29)})
# 36.213 Table 7.1.7.1-1A (common-mode, docstring)
_m = re.search(r"lsn_mcs_dl_256qam\[32\]\[2\]\s*=\s*\{(.*?)\};", _TABLES_SRC, re.S)
MCS_256QAM = {m: (int(a), int(b)) for m, (a, b) in enumerate(re.findall(r"\{(-?\d+),(-?\d+)\}", _m.group(1))) if int(b) >= 0}
# 36.212 5.1.1
G_CRC24A = sum(1 << e for e in (24, 23, 18, 17, 14, 11, 10, 7, 6, 5, 4, 3, 1, 0))
G_CRC24B = sum(1 << e for e in (24, 23, 6, 5, 1, 0))
# 36.212 Table 5.1.4-1: inter-column permutation of the turbo sub-block interleaver (the bit reversal of the five-bit column number)
PERM_TC = (0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30, 1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31)
assert all(PERM_TC[j] == int(format(j, "05b")[::-1], 2) for j in range(32))
NULL = 2   # <NULL> in a uint8 bit stream


def tbs_of(mcs, nof_prb, table256=False):
    """36.213 7.1.7: -> (Q_m, TBS) of an MCS index on N_PRB blocks"""
    qm, itbs = (MCS_256QAM if table256 else MCS_64QAM)[mcs]
    return qm, _TBS_FILE[itbs][nof_prb - 1]


# ---------------------------------------------------------------------------------------------------------------------------- coding (36.212)
def crc24(bits, poly):
    """36.212 5.1.1: parity p_0 .. p_23 of a(D) D^24 mod g(D), p_0 the coefficient of D^23"""
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    v <<= 24
    for s in range(v.bit_length() - 1, 23, -1):
        if (v >> s) & 1:
            v ^= poly << (s - 24)
    return [(v >> (23 - i)) & 1 for i in range(24)]


def segment(A):
    """36.212 5.1.2 for a transport block of A bits (B = A + 24 with its CRC) -> dict(C, Kp, Km, Cp, Cm, F, Ks: the size of each block)"""
    Z, B = 6144, A + 24
    if B <= Z:
        L, C, Bp = 0, 1, B
    else:
        L = 24
        C = -(-B // (Z - L))
        Bp = B + C * L
    Kp = min(k for k in K_SIZES if C * k >= Bp)
    if C == 1:
        Cp, Km, Cm = 1, 0, 0
    else:
        Km = max(k for k in K_SIZES if k < Kp)
        Cm = (C * Kp - Bp) // (Kp - Km)
        Cp = C - Cm
    F = Cp * Kp + Cm * Km - Bp
    return dict(C=C, Kp=Kp, Km=Km, Cp=Cp, Cm=Cm, F=F, L=L, Ks=[Km] * Cm + [Kp] * Cp)


def code_blocks(tb_bits):
    """5.1.1 + 5.1.2: CRC24A on the transport block, F filler bits (<NULL>) in front of the first block, the K- blocks first, CRC24B on every block when
    there are several -> (list of c_r uint8 arrays with NULL fillers, segmentation dict)"""
    b = list(tb_bits) + crc24(tb_bits, G_CRC24A)
    seg = segment(len(tb_bits))
    out, s = [], 0
    for r, K in enumerate(seg["Ks"]):
        F = seg["F"] if r == 0 else 0
        n = K - F - seg["L"]
        data = b[s:s + n]
        s += n
        c = [0] * F + data       # 5.1.2: the filler bits count as 0 in the CRC ...
        if seg["C"] > 1:
            c += crc24(c, G_CRC24B)
        c = np.array(c, dtype=np.uint8)
        c[:F] = NULL             # ... and are <NULL> in c_r
        out.append(c)
    assert s == len(b)
    return out, seg


def _constituent(c):
    """5.1.3.2.1: G(D) = [1, g1 / g0], g0 = 1 + D^2 + D^3, g1 = 1 + D + D^3, from the all-zero state; 5.1.3.2.2: three more steps with the switch
    down, the input being the register feedback -> (z[K] parity, x_tail[3], z_tail[3])"""
    s1 = s2 = s3 = 0
    z = np.zeros(len(c), dtype=np.uint8)
    for k, u in enumerate(c):
        a = int(u) ^ s2 ^ s3
        z[k] = a ^ s1 ^ s3
        s1, s2, s3 = a, s1, s2
    xt, zt = [], []
    for _ in range(3):
        xt.append(s2 ^ s3)      # the input that makes the feedback sum zero
        zt.append(s1 ^ s3)
        s1, s2, s3 = 0, s1, s2
    return z, xt, zt


def qpp(K):
    """5.1.3.2.3: Pi(i) = (f1 i + f2 i^2) mod K"""
    f1, f2 = QPP_F[K]
    i = np.arange(K, dtype=np.int64)
    return (f1 * i + f2 * i * i) % K


def turbo_encode(c):
    """5.1.3.2: c[K] (NULL = filler, encoded as 0) -> d[3, K + 4] with d0, d1 <NULL> on the filler positions; the twelve tail bits in the order of
    5.1.3.2.2: d0 = x_K, z_K+1, x'_K, z'_K+1; d1 = z_K, x_K+2, z'_K, x'_K+2; d2 = x_K+1, z_K+2, x'_K+1, z'_K+2"""
    K = len(c)
    fill = c == NULL
    cc = np.where(fill, 0, c).astype(np.uint8)
    z, xt, zt = _constituent(cc)
    zp, xpt, zpt = _constituent(cc[qpp(K)])
    d = np.zeros((3, K + 4), dtype=np.uint8)
    d[0, :K], d[1, :K], d[2, :K] = cc, z, zp
    d[0, :K][fill] = NULL
    d[1, :K][fill] = NULL
    d[0, K:] = xt[0], zt[1], xpt[0], zpt[1]
    d[1, K:] = zt[0], xt[2], zpt[0], xpt[2]
    d[2, K:] = xt[1], zt[2], xpt[1], zpt[2]
    return d


def circular_buffer(D):
    """5.1.4.1.1 / 5.1.4.1.2 for streams of D bits -> (w: index into the flat d[3 * D] of every circular-buffer position, -1 = a <NULL> of the
    interleaver, R).  Streams 0, 1: y written row by row after N_D = 32 R - D <NULL>s, columns permuted, read column by column; stream 2:
    pi(k) = (P(floor(k / R)) + 32 (k mod R) + 1) mod K_Pi; w_k = v0_k, w_K+2k = v1_k, w_K+2k+1 = v2_k"""
    R = -(-D // 32)
    KP = 32 * R
    ND = KP - D
    k = np.arange(KP)
    col = np.array(PERM_TC)[k // R]
    v01 = col + 32 * (k % R) - ND
    v2 = (col + 32 * (k % R) + 1) % KP - ND
    w = np.full(3 * KP, -1, dtype=np.int64)
    w[:KP] = np.where(v01 >= 0, v01, -1)
    w[KP::2] = np.where(v01 >= 0, D + v01, -1)
    w[KP + 1::2] = np.where(v2 >= 0, 2 * D + v2, -1)
    return w, R


def rate_match(d, E, rv):
    """5.1.4.1.2 with N_cb = K_w: k0 = R (2 ceil(N_cb / (8 R)) rv + 2); E bits from k0 on, cyclically, every <NULL> skipped
    -> (e[E], src[E]: the flat index into d of each e_k)"""
    D = d.shape[1]
    w, R = circular_buffer(D)
    ncb = len(w)
    k0 = R * (2 * (-(-ncb // (8 * R))) * rv + 2)
    flat = d.reshape(-1)
    order = np.roll(w, -k0)
    order = order[order >= 0]
    order = order[flat[order] != NULL]
    src = np.resize(order, E)
    return flat[src].copy(), src


def block_sizes_E(G, C, NL, Qm):
    """5.1.4.1.2: G' = G / (N_L Q_m), gamma = G' mod C; block r gets N_L Q_m floor(G' / C) bits when r <= C - gamma - 1, else N_L Q_m ceil(G' / C)"""
    Gp = G // (NL * Qm)
    gamma = Gp % C
    return [NL * Qm * (Gp // C) if r <= C - gamma - 1 else NL * Qm * (-(-Gp // C)) for r in range(C)]


def encode_tb(tb_bits, G, NL, Qm, rv):
    """one transport block -> dict(f[G]: the codeword after 5.1.5 concatenation, seg, blocks: per block dict(K, F, E, d[3, K + 4], src))"""
    cbs, seg = code_blocks(tb_bits)
    Es = block_sizes_E(G, seg["C"], NL, Qm)
    blocks, f = [], []
    for r, c in enumerate(cbs):
        d = turbo_encode(c)
        e, src = rate_match(d, Es[r], rv)
        blocks.append(dict(K=len(c), F=seg["F"] if r == 0 else 0, E=Es[r], d=d, src=src, e=e))
        f.append(e)
    return dict(f=np.concatenate(f), seg=seg, blocks=blocks, rv=rv)


# ---------------------------------------------------------------------------------------------------------------------------- modulation (36.211 7.1)
def modulate(b, Qm):
    """36.211 7.1.1 - 7.1.5 as closed forms: the first bit pair gives the signs, each further pair folds the amplitude once more:
    16QAM |I| = 2 - s2, 64QAM |I| = 4 - s2 (2 - s4), 256QAM |I| = 8 - s2 (4 - s4 (2 - s6)), with s_n = 1 - 2 b(n); Q the same on the odd bits"""
    s = 1.0 - 2.0 * np.asarray(b, dtype=np.float64).reshape(-1, Qm)
    amp = np.ones((len(s), 2))
    for j in range(Qm // 2 - 1, 0, -1):
        amp = 2.0 ** (Qm // 2 - j) - s[:, 2 * j:2 * j + 2] * amp
    # amp is now |I|, |Q| in odd integers; 7.1: 1/sqrt2, 1/sqrt10, 1/sqrt42, 1/sqrt170 = the root of the mean of the squared odd integers, twice
    norm = np.sqrt(2.0 * np.mean(np.arange(1, 2 ** (Qm // 2), 2) ** 2.0))
    return (s[:, 0] * amp[:, 0] + 1j * s[:, 1] * amp[:, 1]) / norm


# ---------------------------------------------------------------------------------------------------------------------------- layers and precoding (36.211 6.3.3, 6.3.4)
SCHEMES = ("port0", "txd", "cdd", "mux1", "mux2")
CODEBOOK_1L = (1, -1, 1j, -1j)   # 36.211 Table 6.3.4.2.3-1, one layer: [1, q] / sqrt2 for codebook index 0..3


def precode(dcw, scheme, nof_ports, pmi=0):
    """dcw: the modulation symbols of codeword 0 (and 1) -> y[nof_ports, M_ap]
    port0 (6.3.4.1); txd (6.3.3.3 + 6.3.4.3, 2 and 4 ports); cdd (6.3.4.2.2, two layers on two ports: W = I / sqrt2, D(i) = diag(1, e^-j pi i),
    U = [[1, 1], [1, -1]] / sqrt2); mux1 (6.3.4.2.1, one layer, codebook index pmi 0..3); mux2 (two layers, codebook index pmi 1..2:
    [[1, 1], [1, -1]] / 2, [[1, 1], [j, -j]] / 2).  Two codewords on two layers: x0 = d0, x1 = d1 (6.3.3.2)"""
    if scheme in ("port0", "txd"):
        assert scheme == "txd" or nof_ports == 1
        return SD.tx_diversity(dcw[0], nof_ports)
    assert nof_ports == 2
    if scheme == "mux1":
        x = np.asarray(dcw[0])
        return np.stack([x, CODEBOOK_1L[pmi] * x]) / np.sqrt(2.0)
    x0, x1 = np.asarray(dcw[0]), np.asarray(dcw[1])
    assert len(x0) == len(x1)
    if scheme == "cdd":
        alt = np.where(np.arange(len(x0)) % 2 == 0, 1.0, -1.0)    # e^(-j 2 pi i / 2)
        return np.stack([x0 + x1, alt * (x0 - x1)]) / 2.0
    q = {1: 1.0, 2: 1j}[pmi]
    return np.stack([x0 + x1, q * (x0 - x1)]) / 2.0


# ---------------------------------------------------------------------------------------------------------------------------- resource elements (36.211 6.3.5)
def pdsch_res(nof_prb, nof_ports, cell_id, cp, sf_idx, nof_ctrl, prbs):
    """the PDSCH resource elements of the allocated PRBs (the same in both slots) in mapping order: l outer, k inner, from the first symbol after the
    control region; without the CRS of every port of the cell (6.10.1.2), the PBCH block (6.6.4: 72 centre subcarriers, symbols 0-3 of slot 1 of
    subframe 0, including its reserved reference-signal elements) and the PSS / SSS with their guard subcarriers (6.11.1.2 / 6.11.2.2: the 72 centre
    subcarriers of the last two symbols of slots 0 and 10) -> list of (l, k)"""
    nsl = 6 if cp else 7
    rs = SD.crs_positions(cell_id, nof_prb, range(nof_ports), sf_idx, cp)
    centre = range(6 * nof_prb - 36, 6 * nof_prb + 36)
    out = []
    for l in range(nof_ctrl, 2 * nsl):
        blocked = set(rs.get(l, ()))
        if (sf_idx in (0, 5) and l in (nsl - 2, nsl - 1)) or (sf_idx == 0 and nsl <= l < nsl + 4):
            blocked |= set(centre)
        out += [(l, k) for n in sorted(prbs) for k in range(12 * n, 12 * n + 12) if k not in blocked]
    return out


def build(nof_prb, nof_ports, cell_id, cp, sf_idx, nof_ctrl, rnti, prbs, scheme, tbs, pmi=0):
    """one PDSCH.  tbs: per codeword q (in order) dict(bits, Qm, rv).  -> dict(res, y[nof_ports, len(res)], cw: per codeword the encode_tb dict + Qm, G)"""
    res = pdsch_res(nof_prb, nof_ports, cell_id, cp, sf_idx, nof_ctrl, prbs)
    n = len(res)
    NL = 2 if scheme == "txd" else 1        # 5.1.4.1.2: N_L = 2 for transmit diversity, else the layers the block is mapped onto (one each here)
    assert len(tbs) == (2 if scheme in ("cdd", "mux2") else 1)
    cws, syms = [], []
    for q, t in enumerate(tbs):
        G = n * t["Qm"]
        enc = encode_tb(t["bits"], G, NL, t["Qm"], t["rv"])
        # 6.3.1: c_init = n_RNTI 2^14 + q 2^13 + floor(n_s / 2) 2^9 + N_ID
        c = S.gold(rnti * 2 ** 14 + q * 2 ** 13 + sf_idx * 2 ** 9 + cell_id, G)
        syms.append(modulate(enc["f"] ^ c, t["Qm"]))
        enc.update(Qm=t["Qm"], G=G, c=c, bits=np.asarray(t["bits"], dtype=np.uint8))
        cws.append(enc)
    y = precode(syms, scheme, nof_ports, pmi)
    assert y.shape == (nof_ports, n)
    return dict(res=res, y=y, cw=cws, rnti=rnti, scheme=scheme, prbs=sorted(prbs))

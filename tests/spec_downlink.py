"""A downlink control-region transmitter written from TS 36.211 / 36.212 / 36.213 alone, in float64 numpy (test infrastructure only).

It shares no table and no line with the synthetic transmitter (tools/txgen), the oracle (oracle/) or the product: the convolutional sub-block
permutation, the CRC polynomial, the code generators, the PCFICH codewords and the MIB layout are written out again below from the
specifications, with the clause next to each.  It reuses tests/second_frontend.py (Gold sequence 36.211 7.2, CRS 6.10.1, the symbol timing of
Table 6.12-1), which is itself a spec-only derivation.

One call renders one subframe: the CRS of every port, PCFICH, PHICH (random QPSK in every PHICH REG), PDCCH (DCIs at chosen CCEs, every other CCE
filled with random QPSK) and, in subframe 0, the PBCH; through a flat per-(port, rx) gain, optional AWGN and an overall amplitude.  It returns the
waveform and the ground truth.  Two small models go with it: the 36.213 9.1.1 search space with FALCON's ambiguity rule, and a float64 evaluation of
the receiver's REG equaliser (1 port: maximum-ratio combining with the noise in the denominator; 2 ports: SFBC; 4 ports: SFBC-FSTD)."""
from fractions import Fraction

import numpy as np

import second_frontend as S

FFT = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}
BANDWIDTHS = (6, 15, 25, 50, 75, 100)            # 36.331 MasterInformationBlock dl-Bandwidth n6 .. n100 (enumerated 0..5)
PHICH_NG = {1: 0, 3: 1, 6: 2, 12: 3}             # 6 * Ng -> 36.331 phich-Resource oneSixth, half, one, two

# 36.212 Table 5.1.4-2: inter-column permutation of the sub-block interleaver for convolutionally coded channels (also the PDCCH quadruplet
# interleaver, 36.211 6.8.5)
PERM_CC = (1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30)
# 36.212 5.1.1: gCRC16(D) = D^16 + D^12 + D^5 + 1
G_CRC16 = (1 << 16) | (1 << 12) | (1 << 5) | 1
# 36.212 5.1.3.1: rate-1/3 tail-biting convolutional code, constraint length 7, G0 = 133, G1 = 171, G2 = 165 (octal)
G_CONV = (0o133, 0o171, 0o165)
# 36.212 5.3.1.1 Table 5.3.1.1-1: PBCH CRC mask x_ant,0..15 for 1 / 2 / 4 transmit antenna ports
X_ANT = {1: [0] * 16, 2: [1] * 16, 4: [0, 1] * 8}
# 36.212 Table 5.3.4-1: CFI codewords <b0, ..., b31>
CFI_CW = {1: ([0, 1, 1] * 11)[:32], 2: ([1, 0, 1] * 11)[:32], 3: ([1, 1, 0] * 11)[:32]}
# 36.213 9.1.1: Y_k = (A Y_k-1) mod D, Y_-1 = n_RNTI; M(L) candidates of the UE-specific / common spaces
YK_A, YK_D = 39827, 65537
M_UE = {1: 6, 2: 6, 4: 2, 8: 2}
M_COMMON = {4: 4, 8: 2}
SI_RNTI = 0xFFFF


# ---------------------------------------------------------------------------------------------------------------------------- channel coding (36.212)
def crc16(bits):
    """36.212 5.1.1: parity bits p_0 .. p_15 of a(D) D^16 mod gCRC16(D), p_0 the coefficient of D^15"""
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    v <<= 16
    for s in range(v.bit_length() - 1, 15, -1):
        if (v >> s) & 1:
            v ^= G_CRC16 << (s - 16)
    return [(v >> (15 - i)) & 1 for i in range(16)]


def dci_attach_crc(payload, rnti):
    """36.212 5.3.3.2: c_k = a_k; c_A+k = p_k xor x_rnti,k with x_rnti,0 the MSB of the RNTI"""
    x = [(rnti >> (15 - k)) & 1 for k in range(16)]
    return list(payload) + [p ^ r for p, r in zip(crc16(payload), x)]


def conv_encode(c):
    """36.212 5.1.3.1: tail-biting (shift register s_i = c_K-1-i at the start) -> d[3, K]; generator bit 6 taps the input c_k, bit 6-j taps c_k-j"""
    c = np.asarray(c, dtype=np.uint8)
    d = np.zeros((3, len(c)), dtype=np.uint8)
    for s, g in enumerate(G_CONV):
        for j in range(7):
            if (g >> (6 - j)) & 1:
                d[s] ^= np.roll(c, j)  # np.roll(c, j)[k] = c[(k - j) mod K]
    return d


def subblock_cc(D):
    """36.212 5.1.4.2.1: read-out order of the sub-block interleaver for D bits -> index into the input (-1 = <NULL>).  R rows of C = 32
    columns written row by row after N_D = 32 R - D leading <NULL>s, the columns permuted by PERM_CC, read out column by column"""
    R = -(-D // 32)
    nd = 32 * R - D
    return [r * 32 + PERM_CC[j] - nd if r * 32 + PERM_CC[j] >= nd else -1 for j in range(32) for r in range(R)]


def rate_match_cc(d, E):
    """36.212 5.1.4.2: three interleaved streams one after the other (bit collection), then E bits read cyclically, <NULL>s skipped"""
    D = d.shape[1]
    p = subblock_cc(D)
    w = [int(d[s, i]) for s in range(3) for i in p if i >= 0]  # the circular buffer without its <NULL>s: the order is what matters
    return np.array([w[k % len(w)] for k in range(E)], dtype=np.uint8)


def dci_encode(payload, rnti, L):
    """a DCI of len(payload) bits for `rnti` at aggregation level L -> the 72 L bits of its PDCCH"""
    return rate_match_cc(conv_encode(dci_attach_crc(payload, rnti)), 72 * L)


def mib_bits(nof_prb, ng_x6, sfn, phich_extended=0):
    """36.331 MasterInformationBlock: dl-Bandwidth (3), phich-Duration (1), phich-Resource (2), systemFrameNumber (8 MSBs of the SFN), spare (10)"""
    bw, ng, s = BANDWIDTHS.index(nof_prb), PHICH_NG[ng_x6], (sfn >> 2) & 0xFF
    return [(bw >> 2) & 1, (bw >> 1) & 1, bw & 1, phich_extended, (ng >> 1) & 1, ng & 1] + [(s >> (7 - i)) & 1 for i in range(8)] + [0] * 10


def pbch_coded(mib, nof_ports, cp):
    """36.212 5.3.1: CRC16 masked with x_ant, convolutional code, rate matching to 1920 (normal CP) / 1728 (extended CP) bits"""
    c = list(mib) + [p ^ x for p, x in zip(crc16(mib), X_ANT[nof_ports])]
    return rate_match_cc(conv_encode(c), 1728 if cp else 1920)


# ---------------------------------------------------------------------------------------------------------------------------- modulation (36.211)
def qpsk(b):
    """36.211 7.1.2: b(2i), b(2i+1) -> ((1 - 2 b(2i)) + j (1 - 2 b(2i+1))) / sqrt 2"""
    b = np.asarray(b, dtype=np.float64)
    return ((1 - 2 * b[0::2]) + 1j * (1 - 2 * b[1::2])) / np.sqrt(2.0)


def tx_diversity(d, nof_ports):
    """36.211 6.3.3.1 / 6.3.3.3 layer mapping and 6.3.4.1 / 6.3.4.3 precoding -> y[nof_ports, len(d)] (1 port: y = d; 2 ports: SFBC on symbol
    pairs; 4 ports: SFBC-FSTD on quadruplets, the first pair on ports 0 and 2, the second on ports 1 and 3)"""
    d = np.asarray(d, dtype=np.complex128)
    y = np.zeros((nof_ports, len(d)), dtype=np.complex128)
    if nof_ports == 1:
        y[0] = d
        return y
    r = 1 / np.sqrt(2.0)
    if nof_ports == 2:
        x0, x1 = d[0::2], d[1::2]
        y[0, 0::2], y[1, 0::2] = r * x0, -r * np.conj(x1)
        y[0, 1::2], y[1, 1::2] = r * x1, r * np.conj(x0)
        return y
    x0, x1, x2, x3 = d[0::4], d[1::4], d[2::4], d[3::4]
    y[0, 0::4], y[2, 0::4] = r * x0, -r * np.conj(x1)
    y[0, 1::4], y[2, 1::4] = r * x1, r * np.conj(x0)
    y[1, 2::4], y[3, 2::4] = r * x2, -r * np.conj(x3)
    y[1, 3::4], y[3, 3::4] = r * x3, r * np.conj(x2)
    return y


def ofdm_mod(grid, nfft, cp):
    """the inverse of second_frontend.ofdm_demod (36.211 6.12): grid[nsym, nre] -> one subframe of time samples, each symbol led by its cyclic prefix"""
    starts, sflen = S.symbol_starts(nfft, cp)
    nre = grid.shape[1]
    x = np.zeros(sflen, dtype=np.complex128)
    prev = 0
    for i, s in enumerate(starts):
        X = np.zeros(nfft, dtype=np.complex128)
        X[nfft - nre // 2:] = grid[i, :nre // 2]
        X[1:nre // 2 + 1] = grid[i, nre // 2:]
        t = np.fft.ifft(X)
        ncp = s - prev
        x[s - ncp:s] = t[nfft - ncp:]
        x[s:s + nfft] = t
        prev = s + nfft
    return x


# ---------------------------------------------------------------------------------------------------------------------------- resource mapping (36.211)
def crs_positions(cell_id, nof_prb, ports, sf_idx, cp):
    """{symbol: set of k} of the CRS of the given ports"""
    out = {}
    for p in ports:
        for l, k, _ in S.crs(cell_id, nof_prb, p, sf_idx, cp):
            out.setdefault(l, set()).update(int(v) for v in k)
    return out


class ControlRegion:
    """36.211 6.2.4 REGs, 6.7.4 PCFICH, 6.9.3 PHICH, 6.8.5 PDCCH of one cell (any subframe: the REG layout does not depend on it)"""

    def __init__(self, nof_prb, nof_ports, cell_id, cp=0, ng_x6=1):
        self.nof_prb, self.nof_ports, self.cell_id, self.cp, self.ng_x6 = nof_prb, nof_ports, cell_id, cp, ng_x6
        nre = 12 * nof_prb
        # 6.2.4: a single CRS port counts as ports 0 and 1; the REG width follows the CRS in the first slot's symbols
        rs = crs_positions(cell_id, nof_prb, range(max(2, nof_ports)), 0, cp)
        self.rs = {l: rs.get(l, set()) for l in range(4)}
        self.width = {0: 6, 1: 6 if nof_ports == 4 else 4, 2: 4, 3: 6 if cp else 4}
        # 6.7.4: k_bar = (N_sc / 2) (N_ID mod 2 N_RB); REG i at k_bar + floor(i N_RB / 2) N_sc / 2, the additions modulo N_RB N_sc
        kbar = 6 * (cell_id % (2 * nof_prb))
        self.pcfich = [(kbar + (i * nof_prb // 2) * 6) % nre for i in range(4)]
        # 6.9: N_group = ceil(Ng N_RB / 8), twice that with the extended CP, which maps two groups per unit (6.9.3: m' counts mapping units)
        ngroup = int(-(-(Fraction(ng_x6, 6) * nof_prb) // 8))
        # 6.9.3, normal duration: REG n_i = (floor(N_ID n_0 / n_0) + m' + floor(i n_0 / 3)) mod n_0 of the n_0 symbol-0 REGs not used by the PCFICH
        free0 = [k for k in range(0, nre, 6) if k not in self.pcfich]
        n0 = len(free0)
        self.phich = sorted({free0[(cell_id + m + (i * n0) // 3) % n0] for m in range(ngroup) for i in range(3)})
        assert len(self.phich) == 3 * ngroup
        self.ngroup = 2 * ngroup if cp else ngroup

    def nof_symbols(self, cfi):
        """6.7: the control region is CFI symbols long, one more at N_RB <= 10"""
        return cfi + (1 if self.nof_prb <= 10 else 0)

    def reg_res(self, l, k0):
        """the four REs of the REG (k0, l) that carry a quadruplet, in increasing k (6.2.4)"""
        kk = [k for k in range(k0, k0 + self.width[l]) if k not in self.rs[l]]
        assert len(kk) == 4, (l, k0, kk)
        return kk

    def pdcch_regs(self, cfi):
        """6.8.5: REG m' -> (l, k0): k' outer, l' inner, the REGs not assigned to PCFICH / PHICH"""
        used = set(self.pcfich) | set(self.phich)
        return [(l, k) for k in range(12 * self.nof_prb) for l in range(self.nof_symbols(cfi)) if k % self.width[l] == 0 and not (l == 0 and k in used)]

    def quadruplet_regs(self, cfi):
        """CCE-order quadruplet q -> its REG (l, k0): sub-block interleaving of the quadruplets (<NULL>s dropped), cyclic shift by N_ID (6.8.5)"""
        regs = self.pdcch_regs(cfi)
        M = len(regs)
        w = [q for q in subblock_cc(M) if q >= 0]
        out = [None] * M
        for m in range(M):
            out[w[(m + self.cell_id) % M]] = regs[m]
        return out

    def nof_cce(self, cfi):
        return len(self.pdcch_regs(cfi)) // 9


def pbch_res(nof_prb, cell_id, cp):
    """36.211 6.6.4: the PBCH REs of subframe 0 in mapping order: symbols 0-3 of slot 1 (l outer), the 72 centre subcarriers (k inner),
    the CRS positions of four ports left out whatever the cell's port count -> list of (symbol in the subframe, k)"""
    nsymb = 6 if cp else 7
    rs = crs_positions(cell_id, nof_prb, range(4), 0, cp)
    k0 = 6 * nof_prb - 36
    return [(nsymb + l, k) for l in range(4) for k in range(k0, k0 + 72) if k not in rs.get(nsymb + l, set())]


# ---------------------------------------------------------------------------------------------------------------------------- one subframe
def control_subframe(nof_prb, nof_ports, cell_id, cp=0, sf_idx=0, sfn=0, cfi=1, ng_x6=1, nof_rx=1, dcis=(), gains=None, snr_db=None, scale=1.0,
                     seed=0, pdsch=()):
    """dcis: (L, ncce, rnti, payload bits).  gains[nof_ports, nof_rx]: flat channel (default: random, |h| in [0.5, 1.5]).
    pdsch: the shared channels of tests/spec_pdsch.py (dicts with res: the (l, k) of their resource elements in mapping order, y[nof_ports, len(res)]),
    placed into the same grid; every other element of the data region stays empty.
    -> (iq[nof_rx, 15 N] complex64, truth dict)"""
    rng = np.random.default_rng(seed)
    nre, nfft, nsym = 12 * nof_prb, FFT[nof_prb], 12 if cp else 14
    reg = ControlRegion(nof_prb, nof_ports, cell_id, cp, ng_x6)
    tx = np.zeros((nof_ports, nsym, nre), dtype=np.complex128)

    def put_quadruplets(quads, places):
        """quads[nof_ports, n, 4] onto REGs (l, k0)"""
        for q, (l, k0) in enumerate(places):
            for p in range(nof_ports):
                tx[p, l, reg.reg_res(l, k0)] = quads[p, q]

    # CRS (6.10.1)
    for p in range(nof_ports):
        for l, k, r in S.crs(cell_id, nof_prb, p, sf_idx, cp):
            tx[p, l, k] = r
    # PCFICH (6.7): codeword, scrambling c_init = (floor(ns/2) + 1)(2 N_ID + 1) 2^9 + N_ID, QPSK, transmit diversity, four REGs of symbol 0
    b = np.array(CFI_CW[cfi], dtype=np.uint8) ^ S.gold((sf_idx + 1) * (2 * cell_id + 1) * 512 + cell_id, 32)
    put_quadruplets(tx_diversity(qpsk(b), nof_ports).reshape(nof_ports, 4, 4), [(0, k) for k in reg.pcfich])
    # PHICH: random non-zero QPSK in every PHICH REG
    put_quadruplets(tx_diversity(qpsk(rng.integers(0, 2, 8 * len(reg.phich))), nof_ports).reshape(nof_ports, -1, 4), [(0, k) for k in reg.phich])
    # PDCCH (6.8): CCE n = bits 72 n .. 72 n + 71; the REGs after the last whole CCE carry <NIL> (zero power)
    places = reg.quadruplet_regs(cfi)
    ncce = len(places) // 9
    bits = rng.integers(0, 2, 72 * ncce).astype(np.uint8)
    taken = np.zeros(ncce, dtype=bool)
    for L, n, rnti, payload in dcis:
        assert n % L == 0 and n + L <= ncce and not taken[n:n + L].any(), (L, n, ncce)
        taken[n:n + L] = True
        bits[72 * n:72 * (n + L)] = dci_encode(payload, rnti, L)
    c = S.gold(sf_idx * 512 + cell_id, 8 * len(places))  # c_init = floor(ns/2) 2^9 + N_ID
    d = np.zeros(4 * len(places), dtype=np.complex128)
    d[:36 * ncce] = qpsk(bits ^ c[:72 * ncce])
    put_quadruplets(tx_diversity(d, nof_ports).reshape(nof_ports, -1, 4), places)
    truth = dict(cfi=cfi, nof_cce=ncce, pdcch_bits=bits, dcis=list(dcis), regs=places, reg=reg)
    # PBCH (6.6) in subframe 0: quarter sfn mod 4 of the scrambled 40 ms block
    if sf_idx == 0:
        mib = mib_bits(nof_prb, ng_x6, sfn)
        e = pbch_coded(mib, nof_ports, cp)
        E4 = len(e) // 4
        q = sfn % 4
        quarter = (e ^ S.gold(cell_id, len(e)))[E4 * q:E4 * (q + 1)]
        y = tx_diversity(qpsk(quarter), nof_ports)
        for i, (l, k) in enumerate(pbch_res(nof_prb, cell_id, cp)):
            tx[:, l, k] = y[:, i]
        truth.update(mib=mib, pbch_bits=quarter)
    # PDSCH (6.3.5): nothing may land on an element that is in use
    for ch in pdsch:
        ll, kk = np.array([l for l, _ in ch["res"]]), np.array([k for _, k in ch["res"]])
        assert ll.min() >= reg.nof_symbols(cfi) and not np.any(tx[:, ll, kk]), "PDSCH on an occupied resource element"
        tx[:, ll, kk] = ch["y"]
    truth["pdsch"] = list(pdsch)
    # channel: a flat complex gain per (port, rx), AWGN of variance 10^(-snr/10) per RE, an overall amplitude
    if gains is None:
        gains = rng.uniform(0.5, 1.5, (nof_ports, nof_rx)) * np.exp(2j * np.pi * rng.uniform(0, 1, (nof_ports, nof_rx)))
    iq = np.zeros((nof_rx, 15 * nfft), dtype=np.complex128)
    for rx in range(nof_rx):
        iq[rx] = ofdm_mod(np.tensordot(gains[:, rx], tx, axes=1), nfft, cp)
        if snr_db is not None:
            sd = np.sqrt(10 ** (-snr_db / 10) / nfft / 2)  # the unnormalised FFT of the receiver multiplies the per-sample variance by N
            iq[rx] += sd * (rng.standard_normal(iq.shape[1]) + 1j * rng.standard_normal(iq.shape[1]))
    truth["gains"] = gains
    return (scale * iq).astype(np.complex64), truth


# ---------------------------------------------------------------------------------------------------------------------------- the two models
def search_space(nof_cce, rnti, sf_idx):
    """36.213 9.1.1 locations {(L, first CCE)} FALCON searches for `rnti`: RA-RNTI (1..10) and M/P/SI-RNTI (>= 0xFFFD) the common space, a C-RNTI
    (0x000B..0xFFF3) its UE-specific space (Y_-1 = n_RNTI, k = floor(ns/2)) and the common space, anything else nothing"""
    locs = set()
    if 1 <= rnti <= 0xFFF3 or rnti >= 0xFFFD:
        for L, M in M_COMMON.items():
            if nof_cce // L:
                locs |= {(L, L * (m % (nof_cce // L))) for m in range(M)}
    if 0x000B <= rnti <= 0xFFF3:
        Y = rnti
        for _ in range(sf_idx + 1):
            Y = (YK_A * Y) % YK_D
        for L, M in M_UE.items():
            if nof_cce // L:
                locs |= {(L, L * ((Y + m) % (nof_cce // L))) for m in range(M)}
    return locs


def validate_location(nof_cce, ncce, L, sf_idx, rnti):
    """FALCON's verdict on a decoded location (falcon_pdcch.c:223-250): 0 not in the search space of the RNTI, 1 in it but also a candidate of level
    L / 2 at the same first CCE (ambiguous), 2 valid"""
    locs = search_space(nof_cce, rnti, sf_idx)
    if (L, ncce) not in locs:
        return 0
    return 1 if L > 1 and (L // 2, ncce) in locs else 2


def equalise(grid, ce, noise, nof_ports, places_res):
    """float64 evaluation of the receiver's REG equaliser on its own inputs.  grid[rx, sym, k], ce[port, rx, sym, k], places_res: list of (l, kk[4]).
    -> (x[n, 4] complex128, mag[n, 4]: the sum of the magnitudes of the terms each x is made of, the scale of its rounding error).
    1 port: x = sum_rx y conj(h) / (sum_rx |h|^2 + noise); 2 ports (SFBC) / 4 ports (SFBC-FSTD, pairs on ports (0, 2) then (1, 3)):
    x0 = sqrt2 sum_rx (conj(h_a,k) r_k + h_b,k+1 conj(r_k+1)) / sum_rx (|h_a,k|^2 + |h_b,k+1|^2), x1 = sqrt2 sum_rx (conj(h_a,k+1) r_k+1 - h_b,k conj(r_k)) / (same)"""
    g = grid.astype(np.complex128)
    h = ce.astype(np.complex128)
    n = len(places_res)
    x = np.zeros((n, 4), dtype=np.complex128)
    mag = np.zeros((n, 4))
    for q, (l, kk) in enumerate(places_res):
        if nof_ports == 1:
            y, hh = g[:, l, kk], h[0][:, l, kk]
            den = np.sum(np.abs(hh) ** 2, axis=0) + noise
            x[q] = np.sum(y * np.conj(hh), axis=0) / den
            mag[q] = np.sum(np.abs(y * hh), axis=0) / den + np.abs(x[q])
            continue
        for i in (0, 2):
            pa = 1 if (nof_ports == 4 and i == 2) else 0
            pb = pa + 2 if nof_ports == 4 else 1
            r0, r1 = g[:, l, kk[i]], g[:, l, kk[i + 1]]
            h00, h01, h10, h11 = h[pa][:, l, kk[i]], h[pa][:, l, kk[i + 1]], h[pb][:, l, kk[i]], h[pb][:, l, kk[i + 1]]
            den = np.sum(np.abs(h00) ** 2 + np.abs(h11) ** 2)
            t0 = np.sum(np.conj(h00) * r0 + h11 * np.conj(r1))
            t1 = np.sum(np.conj(h01) * r1 - h10 * np.conj(r0))
            x[q, i], x[q, i + 1] = np.sqrt(2) * t0 / den, np.sqrt(2) * t1 / den
            m0 = np.sum(np.abs(h00 * r0) + np.abs(h11 * r1))
            m1 = np.sum(np.abs(h01 * r1) + np.abs(h10 * r0))
            mag[q, i] = np.sqrt(2) * m0 / den + np.abs(x[q, i])
            mag[q, i + 1] = np.sqrt(2) * m1 / den + np.abs(x[q, i + 1])
    return x, mag


def pdcch_llr_model(grid, ce, noise, reg, cfi, sf_idx):
    """the PDCCH soft bits in CCE order from the float64 equaliser: LLR = -sqrt2 Re x / -sqrt2 Im x, descrambled (positive = bit 1)
    -> (llr[72 nof_cce], mag[72 nof_cce]: the rounding scale of each, same units)"""
    places = reg.quadruplet_regs(cfi)
    ncce = len(places) // 9
    x, mag = equalise(grid, ce, noise, reg.nof_ports, [(l, reg.reg_res(l, k0)) for l, k0 in places[:9 * ncce]])
    llr = np.empty(72 * ncce)
    llr[0::2], llr[1::2] = -np.sqrt(2) * x.real.ravel(), -np.sqrt(2) * x.imag.ravel()
    m = np.repeat(np.sqrt(2) * mag.ravel(), 2)
    c = S.gold(sf_idx * 512 + reg.cell_id, 72 * ncce).astype(bool)
    llr[c] = -llr[c]
    return llr, m

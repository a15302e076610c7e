"""DCI payloads of formats 0, 1A, 1, 2A and 2 for FDD, packed from TS 36.212 5.3.3.1 and TS 36.213 7.1.6 / 8.4 alone (test infrastructure only; no line
shared with tools/txgen, oracle/ or the product).

Covered: the field order of each format, resource allocation type 0 (RBG size P of 36.213 Table 7.1.6.1-1, the short last RBG), type 2 with
localised VRBs (the RIV of 7.1.6.3), the type-0 / type-1 header bit above 10 PRB, the transport-block-to-codeword swap flag, the precoding information
field for two ports (36.212 Table 5.3.3.1.5-4; format 2A has none on two ports, Table 5.3.3.1.5A-1), the hopping bits of format 0 (36.213 Table 8.4-1)
and the size rules of 5.3.3.1.
Left out: resource allocation type 1 and distributed VRBs (nothing here packs them)."""
AMBIGUOUS = (12, 14, 16, 20, 24, 26, 32, 40, 44, 56)     # 36.212 Table 5.3.3.1.2-1


def _bits(v, n):
    assert 0 <= v < (1 << n) or n == 0 and v == 0, (v, n)
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def clog2(x):
    return (x - 1).bit_length()


def rbg_size(nof_prb):
    """36.213 Table 7.1.6.1-1"""
    return 1 if nof_prb <= 10 else 2 if nof_prb <= 26 else 3 if nof_prb <= 63 else 4


def riv_bits(nof_prb):
    """5.3.3.1.3: ceil(log2(N_RB (N_RB + 1) / 2))"""
    return clog2(nof_prb * (nof_prb + 1) // 2)


def riv(nof_prb, start, length):
    """36.213 7.1.6.3: RIV = N (L - 1) + RB_start when L - 1 <= floor(N / 2), else N (N - L + 1) + (N - 1 - RB_start)"""
    assert length >= 1 and start + length <= nof_prb
    if length - 1 <= nof_prb // 2:
        return nof_prb * (length - 1) + start
    return nof_prb * (nof_prb - length + 1) + (nof_prb - 1 - start)


def type0_field(nof_prb, rbgs):
    """36.213 7.1.6.1: bitmap of ceil(N / P) bits, RBG 0 at the MSB; behind the header bit (0 = type 0) when N > 10 (36.212 5.3.3.1.2)
    -> (bits, the PRBs of those RBGs: the last RBG has N - P floor(N / P) blocks when P does not divide N)"""
    P = rbg_size(nof_prb)
    n = -(-nof_prb // P)
    assert all(0 <= g < n for g in rbgs)
    bits = ([0] if nof_prb > 10 else []) + [1 if g in rbgs else 0 for g in range(n)]
    prbs = [p for g in sorted(rbgs) for p in range(g * P, min((g + 1) * P, nof_prb))]
    return bits, prbs


def size_format0(nof_prb):
    """5.3.3.1.1, FDD, one uplink carrier: flag, hopping, RIV, MCS/RV 5, NDI, TPC 2, DM-RS shift 3, CSI request 1; padded to format 1A"""
    return max(1 + 1 + riv_bits(nof_prb) + 5 + 1 + 2 + 3 + 1, size_format1a(nof_prb))


def size_format1a(nof_prb):
    """5.3.3.1.3: flag, localised/distributed, RIV, MCS 5, HARQ 3, NDI, RV 2, TPC 2; zeros until the size of format 0; one more zero when the size
    is one of Table 5.3.3.1.2-1"""
    s = max(1 + 1 + riv_bits(nof_prb) + 5 + 3 + 1 + 2 + 2, 1 + 1 + riv_bits(nof_prb) + 5 + 1 + 2 + 3 + 1)
    return s + 1 if s in AMBIGUOUS else s


def _raw_alloc01(nof_prb):
    return (1 if nof_prb > 10 else 0) + -(-nof_prb // rbg_size(nof_prb))


def size_format1(nof_prb):
    """5.3.3.1.2: header, bitmap, MCS 5, HARQ 3, NDI, RV 2, TPC 2; one zero when the size equals format 0 / 1A, and zeros until the size is neither
    ambiguous nor that of format 0 / 1A"""
    s = _raw_alloc01(nof_prb) + 5 + 3 + 1 + 2 + 2
    while s in AMBIGUOUS or s == size_format1a(nof_prb):
        s += 1
    return s


def precoding_bits(fmt, nof_ports):
    """Table 5.3.3.1.5-3 (format 2: 3 bits on two ports, 6 on four) / Table 5.3.3.1.5A-1 (format 2A: none on two ports, 2 on four)"""
    return {("2", 2): 3, ("2", 4): 6, ("2A", 2): 0, ("2A", 4): 2}[(fmt, nof_ports)]


def size_format2x(fmt, nof_prb, nof_ports):
    """5.3.3.1.5 / 5.3.3.1.5A: header, bitmap, TPC 2, HARQ 3, swap flag, (MCS 5, NDI, RV 2) twice, precoding information; one zero when ambiguous"""
    s = _raw_alloc01(nof_prb) + 2 + 3 + 1 + 2 * 8 + precoding_bits(fmt, nof_ports)
    return s + 1 if s in AMBIGUOUS else s


def sizeof(fmt, nof_prb, nof_ports):
    return {"0": size_format0, "1A": size_format1a, "1": size_format1}[fmt](nof_prb) if fmt in ("0", "1A", "1") else size_format2x(fmt, nof_prb, nof_ports)


def _pad(bits, n):
    assert len(bits) <= n, (len(bits), n)
    return bits + [0] * (n - len(bits))


def pack_1a(nof_prb, start, length, mcs, rv, harq=0, ndi=0, tpc=0):
    """format 1A with a C-RNTI, localised VRBs -> (bits, PRBs)"""
    b = [1, 0] + _bits(riv(nof_prb, start, length), riv_bits(nof_prb)) + _bits(mcs, 5) + _bits(harq, 3) + [ndi] + _bits(rv, 2) + _bits(tpc, 2)
    return _pad(b, size_format1a(nof_prb)), list(range(start, start + length))


def hop_bits_format0(nof_prb):
    """36.213 Table 8.4-1: N_UL_hop = 1 for 6..49 PRB, 2 for 50..110"""
    return 1 if nof_prb < 50 else 2


def pack_0(nof_prb, start, length, mcs, ndi=0, tpc=0, cyclic_shift=0, cqi_request=0, hop=None):
    """format 0 (5.3.3.1.1, FDD, one uplink carrier): flag 0, hopping flag, resource block assignment and hopping allocation of
    ceil(log2(N (N + 1) / 2)) bits - with the hopping flag set its N_UL_hop most significant bits are the hopping bits `hop` and the rest carries the
    RIV (36.213 8.4) -, MCS and redundancy version 5, NDI, TPC 2, cyclic shift for DM RS 3, CQI request; zeros up to the size of format 1A -> bits"""
    nb = riv_bits(nof_prb)
    if hop is None:
        alloc = _bits(riv(nof_prb, start, length), nb)
    else:
        nh = hop_bits_format0(nof_prb)
        alloc = _bits(hop, nh) + _bits(riv(nof_prb, start, length), nb - nh)
    b = [0, 0 if hop is None else 1] + alloc + _bits(mcs, 5) + [ndi] + _bits(tpc, 2) + _bits(cyclic_shift, 3) + [cqi_request]
    return _pad(b, size_format0(nof_prb))


def pack_1a_si(nof_prb, start, length, itbs, rv, nprb1a):
    """format 1A with the CRC scrambled by SI-RNTI (5.3.3.1.3): HARQ process and NDI reserved, the MSB of the TPC field reserved, its LSB the column
    N_PRB^1A of the TBS table (0 -> 2, 1 -> 3); the MCS field is I_TBS (36.213 7.1.7.2), the modulation QPSK (7.1.7.1) -> (bits, PRBs)"""
    b = [1, 0] + _bits(riv(nof_prb, start, length), riv_bits(nof_prb)) + _bits(itbs, 5) + [0, 0, 0] + [0] + _bits(rv, 2) + [0, {2: 0, 3: 1}[nprb1a]]
    return _pad(b, size_format1a(nof_prb)), list(range(start, start + length))


def pack_1(nof_prb, rbgs, mcs, rv, harq=0, ndi=0, tpc=0):
    a, prbs = type0_field(nof_prb, rbgs)
    return _pad(a + _bits(mcs, 5) + _bits(harq, 3) + [ndi] + _bits(rv, 2) + _bits(tpc, 2), size_format1(nof_prb)), prbs


def pack_2x(fmt, nof_prb, nof_ports, rbgs, tb1, tb2, swap=0, pinfo=0, harq=0, tpc=0):
    """formats 2 / 2A.  tb1, tb2: (mcs, rv, ndi); a disabled block is (0, 1, ndi) (5.3.3.1.5: I_MCS = 0 and rv_idx = 1)"""
    a, prbs = type0_field(nof_prb, rbgs)
    b = a + _bits(tpc, 2) + _bits(harq, 3) + [swap]
    for mcs, rv, ndi in (tb1, tb2):
        b += _bits(mcs, 5) + [ndi] + _bits(rv, 2)
    b += _bits(pinfo, precoding_bits(fmt, nof_ports))
    return _pad(b, size_format2x(fmt, nof_prb, nof_ports)), prbs


def precoding_info_2ports(nof_codewords, scheme, pmi=0):
    """Table 5.3.3.1.5-4 (format 2, two ports).  One codeword: 0 transmit diversity, 1..4 one layer with codebook index 0..3; two codewords:
    0, 1 two layers with codebook index 1, 2"""
    if nof_codewords == 1:
        return 0 if scheme == "txd" else 1 + pmi
    return pmi - 1

"""The symbol transform of k_ofdm and k_ul_fft at every symbol size, word for word.  The schedule (first pass on registers from the time samples, swizzled
LDS image, last pass straight to the grid row, PRB power from the carriers on chip; lsn_fft_map.h) must not change one bit of the grid: 128 .. 2048 and
1536 against the oracle's o_fft, 384 and 768 against the three-way formula of lsn_dsp.h restated in numpy float32 on top of o_fft(128 / 256) (that
restatement at M = 512 is o_fft(1536): tests/test_fft_schedule.py).  Each case pushes two subframes: receiver noise, then one impulse per symbol at a
different position each with two symbols of zeros (+0 and -0) - the inputs that show a wrong index or a lost sign.  Normal and extended CP, one and two
antennas, a fixed CFO correction (the NCO feeds the register-first loads), the uplink transform, and TAP_RB_POWER against the oracle's o_subframe_power."""
import ctypes as C
import math

import numpy as np
import pytest

import ltesniffer_amd as la
from lsn_testlib import OCell, oracle
from rate_convert import SYMBOL_SZ_3GPP, SYMBOL_SZ_SRSRAN, symbol_starts
from srs_streams import _cmul32, dl_bins, o_fft, ul_bins

pytestmark = pytest.mark.gpu
SIZES = [(la.RATES_3GPP, n) for n in (6, 15, 25, 50, 75, 100)] + [(la.RATES_SRSRAN, n) for n in (25, 50, 75, 100)]
IDS = ["%s-%dprb" % ("3gpp" if r == la.RATES_3GPP else "srsran", n) for r, n in SIZES]
ZERO_SYMBOLS = (5, 10)   # no reference signal of any port lies in them, with either cyclic prefix


def _size(rates, nof_prb):
    return (SYMBOL_SZ_3GPP if rates == la.RATES_3GPP else SYMBOL_SZ_SRSRAN)[nof_prb]


def _circle(N):
    """exp(-2 pi i k / N) as the host builds the table of the radix-3 combination: double angle, libm, rounded to float32"""
    return np.array([complex(np.float32(math.cos(2.0 * math.pi * k / N)), np.float32(-math.sin(2.0 * math.pi * k / N))) for k in range(N)], dtype=np.complex64)


_T = {}


def _pack(re, im):
    """complex64 from float32 parts, the sign of a zero kept (re + 1j * im would lose the sign of a negative-zero real part)"""
    out = np.empty(np.shape(re), dtype=np.complex64)
    out.real, out.imag = re, im
    return out


def _rotated(x, table):
    """x * table, one float32 rounding per operation.  (srs_streams.nco_rotate and ul_shift do the same but join the parts with re + 1j * im, which is
    wrong by the sign of a zero on the all-zero symbols used here; the tables below are the oracle's own, as those helpers fetch them.)"""
    return _pack(*_cmul32(x.real, x.imag, table.real, table.imag))


def _nco_table(pos, cfo_hz, N):
    """o_ofdm_rx's rotation of the N useful samples that start at sample pos of their subframe"""
    lib = oracle()
    lib.o_nco_dphi.restype = C.c_uint32
    lib.o_nco_dphi.argtypes = [C.c_float, C.c_int]
    dphi = int(lib.o_nco_dphi(float(cfo_hz), int(N)))
    coarse, fine = np.zeros(4096, dtype=np.complex64), np.zeros(1024, dtype=np.complex64)
    lib.o_nco_tables.argtypes = [C.c_void_p, C.c_void_p]
    lib.o_nco_tables(coarse.ctypes.data, fine.ctypes.data)
    ph = ((pos + np.arange(N, dtype=np.uint64)) * dphi) & 0xFFFFFFFF
    return _rotated(coarse[(ph >> 20).astype(np.int64)], fine[((ph >> 10) & 1023).astype(np.int64)])


def _ul_table(N):
    t = np.zeros(N, dtype=np.complex64)
    oracle().o_ul_shift_table.argtypes = [C.c_int, C.c_void_p]
    oracle().o_ul_shift_table(int(N), t.ctypes.data)
    return t


def _transform(x):
    """the transform the product must equal: o_fft where the oracle has the size, else X[k] = (F_0[k % M] + F_1[k % M] T[k]) + F_2[k % M] T[2 k mod N]"""
    N = x.shape[-1]
    if N not in (384, 768):
        return o_fft(x)
    M = N // 3
    T = _T.setdefault(N, _circle(N))
    F = [o_fft(np.ascontiguousarray(x[r::3])) for r in range(3)]
    k = np.arange(N)
    kq = k % M
    t1 = _cmul32(F[1][kq].real, F[1][kq].imag, T[k].real, T[k].imag)
    t2 = _cmul32(F[2][kq].real, F[2][kq].imag, T[(2 * k) % N].real, T[(2 * k) % N].imag)
    sr, si = F[0][kq].real + t1[0], F[0][kq].imag + t1[1]
    return _pack(sr + t2[0], si + t2[1])


def _input(N, cp, nant, seed):
    """[2, nant, 15 N]: subframe 0 noise; subframe 1 an impulse per symbol (in the useful part, a different sample each, both signs) and two zero symbols"""
    rng = np.random.default_rng(seed)
    x = np.zeros((2, nant, 15 * N), dtype=np.complex64)
    x[0] = (rng.standard_normal((nant, 15 * N)) + 1j * rng.standard_normal((nant, 15 * N))).astype(np.complex64) * np.float32(0.7)
    at = [0, 1, N // 2, N - 1, N // 8 + 1, 3, N // 2 - 1, N // 4 + 5, 7 * N // 8 + 2, N - 2, 17, N // 2 + 1, 2, N - 9]
    for a in range(nant):
        for l, (p, c) in enumerate(symbol_starts(N, cp)):
            if l == ZERO_SYMBOLS[0]:
                continue
            if l == ZERO_SYMBOLS[1]:
                x[1, a, p:p + c + N] = np.complex64(complex(-0.0, -0.0))
                continue
            x[1, a, p + c + (at[l] + 5 * a) % N] = (1.0 - 0.5j) * (-1.0) ** (l + a)
    return x


def _phy(rates, nof_prb, nant, cp):
    phy = la.Phy(nof_rx_antennas=nant, max_batch=2, pcapwriter=la.PcapWriter(None))
    assert phy.set_sampling(rates)
    assert phy.setCell(nof_prb, 1, 3, cp=cp)
    return phy


@pytest.mark.parametrize("cp,nant,cfo", [(0, 1, 0.0), (1, 2, 0.0), (0, 2, 1234.5)], ids=["normal-1rx", "extended-2rx", "normal-2rx-cfo"])
@pytest.mark.parametrize("rates,nof_prb", SIZES, ids=IDS)
def test_downlink_grid_and_prb_power_equal_the_oracle_word_for_word(rates, nof_prb, cp, nant, cfo):
    N, nre = _size(rates, nof_prb), 12 * nof_prb
    x = _input(N, cp, nant, 100 * nof_prb + N + cp)
    phy = _phy(rates, nof_prb, nant, cp)
    if cfo:
        phy.setCfoCorrection(la.Phy.CFO_FIXED, cfo)
    phy.process_host(x, 0)
    lib = oracle()
    lib.o_subframe_power.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ocell = OCell(nof_prb, 1, 3, 1)
    ndiff, npow = 0, 0
    for sf in range(2):
        g = phy.tap(la.TAP_GRID, sf, np.complex64, nant * 14 * nre).reshape(nant, 14, nre)
        ref = np.zeros((nant, 14, nre), dtype=np.complex64)
        for rx in range(nant):
            for l, (p, c) in enumerate(symbol_starts(N, cp)):
                s = x[sf, rx, p + c:p + c + N]
                if cfo:
                    s = _rotated(s, _nco_table(p + c, cfo, N))
                ref[rx, l] = _transform(s)[dl_bins(N, nre)]
        nsym = 12 if cp else 14
        ndiff += int(np.count_nonzero(g[:, :nsym].view(np.uint32) != ref[:, :nsym].view(np.uint32)))
        want = np.zeros(nof_prb, dtype=np.float32)
        lib.o_subframe_power(C.addressof(ocell), ref[0].ctypes.data, want.ctypes.data, None, None)
        rbp = phy.tap(la.TAP_RB_POWER, sf, np.float32, 110)[:nof_prb]
        npow += int(np.count_nonzero(rbp.view(np.uint32) != want.view(np.uint32)))
    phy.close()
    print("N = %d: %d differing grid words, %d differing PRB powers" % (N, ndiff, npow))
    assert ndiff == 0 and npow == 0, (ndiff, npow)


@pytest.mark.parametrize("cp", [0, 1], ids=["normal", "extended"])
@pytest.mark.parametrize("rates,nof_prb", SIZES, ids=IDS)
def test_uplink_grid_equals_the_oracle_word_for_word(rates, nof_prb, cp):
    N, nre = _size(rates, nof_prb), 12 * nof_prb
    x = _input(N, cp, 1, 7 * nof_prb + N + cp)[:, 0]
    phy = _phy(rates, nof_prb, 1, cp)
    assert phy.setUlConfig(3, 5)
    phy.pusch_decode(x, 0, [])
    ndiff = 0
    for sf in range(2):
        g = phy.tap_ul_grid(sf)
        for l, (p, c) in enumerate(symbol_starts(N, cp)):
            ref = _transform(_rotated(x[sf, p + c:p + c + N], _ul_table(N)))[ul_bins(N, nre)]
            ndiff += int(np.count_nonzero(g[l].view(np.uint32) != ref.view(np.uint32)))
    phy.close()
    print("N = %d: %d differing uplink grid words" % (N, ndiff))
    assert ndiff == 0, ndiff

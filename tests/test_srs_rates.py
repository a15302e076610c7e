"""Sampling modes (LSN_RATES_3GPP / LSN_RATES_SRSRAN), the part that needs no GPU: the symbol-size table of the C ABI, the exported symbols, the
float64 rate converter the GPU tests rely on (tests/rate_convert.py), and the condition the record comparison of the GPU tests rests on - no code block of
the compared streams is decided in the last allowed turbo iteration."""
import numpy as np
import pytest

import ltesniffer_amd as la
from rate_convert import SYMBOL_SZ_3GPP, SYMBOL_SZ_SRSRAN, convert_prach_subframe, convert_subframes, convert_symbol, symbol_starts
from srs_streams import STREAMS, dl_bins, edge_blocks, failed_records, oracle_fft1536_error, stream, ul_bins

PRBS = (6, 15, 25, 50, 75, 100)


def test_symbol_size_and_sampling_rate_tables():
    assert (la.RATES_3GPP, la.RATES_SRSRAN) == (0, 1)
    assert [la.symbol_sz(p, la.RATES_3GPP) for p in PRBS] == [128, 256, 512, 1024, 1536, 2048]
    assert [la.symbol_sz(p, la.RATES_SRSRAN) for p in PRBS] == [128, 256, 384, 768, 1024, 1536]
    assert [la.sampling_freq_hz(p, la.RATES_SRSRAN) for p in PRBS] == [1920000, 3840000, 5760000, 11520000, 15360000, 23040000]
    assert [la.sampling_freq_hz(p, la.RATES_3GPP) for p in PRBS] == [1920000, 3840000, 7680000, 15360000, 23040000, 30720000]
    for bad_prb in (0, 7, 20, 110):
        for r in (0, 1):
            assert la.symbol_sz(bad_prb, r) == 0 and la.sampling_freq_hz(bad_prb, r) == 0
    for bad_mode in (2, -1, 100):
        for p in PRBS:
            assert la.symbol_sz(p, bad_mode) == 0 and la.sampling_freq_hz(p, bad_mode) == 0
    assert {p: la.symbol_sz(p, 0) for p in PRBS} == SYMBOL_SZ_3GPP and {p: la.symbol_sz(p, 1) for p in PRBS} == SYMBOL_SZ_SRSRAN


def test_new_symbols_are_exported():
    for s in ("lsn_phy_set_sampling", "lsn_phy_get_sampling", "lsn_symbol_sz", "lsn_sampling_freq_hz", "lsn_cell_search_rates"):
        assert s in la.EXPORTS
        getattr(la.lib(), s)


def test_cyclic_prefix_lengths_are_whole_numbers_at_every_size():
    for N in (384, 768, 1024, 1536):
        assert (160 * N) % 2048 == 0 and (144 * N) % 2048 == 0 and N % 4 == 0 and (3168 * N) % 2048 == 0
        for cp in (0, 1):
            st = symbol_starts(N, cp)
            assert st[-1][0] + st[-1][1] + N == 15 * N


@pytest.mark.parametrize("nof_prb", [25, 50, 75, 100])
@pytest.mark.parametrize("cp", [0, 1])
def test_converter_keeps_every_occupied_bin(nof_prb, cp):
    """the N_r-point DFT of a converted symbol equals the N-point DFT of the original on every kept bin - occupied carriers and noise alike - to 1e-9
    relative, downlink and uplink (half-carrier shift), on unit-power carriers with noise over the whole band"""
    N, Nr, nre = SYMBOL_SZ_3GPP[nof_prb], SYMBOL_SZ_SRSRAN[nof_prb], 12 * nof_prb
    rng = np.random.default_rng(nof_prb + cp)
    x = np.zeros((2, 15 * N), dtype=np.complex128)
    shift, shift_r = np.exp(-1j * np.pi * np.arange(N) / N), np.exp(-1j * np.pi * np.arange(Nr) / Nr)
    for p, c in symbol_starts(N, cp):
        for a, bins in ((0, dl_bins(N, nre)), (1, ul_bins(N, nre))):
            X = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * 0.05   # noise on every bin of the 3GPP-rate band
            X[bins] += np.exp(2j * np.pi * rng.random(nre))
            s = np.fft.ifft(X)
            if a == 1:
                s = s * np.conj(shift)   # the transmitter's +7.5 kHz
            x[a, p + c:p + c + N] = s
            x[a, p:p + c] = s[N - c:]
    y = convert_subframes(x, nof_prb, cp=cp, uplink_antennas=(1,), dtype=None)
    assert y.shape == (2, 15 * Nr)
    worst = 0.0
    for (p, c), (pr, cr) in zip(symbol_starts(N, cp), symbol_starts(Nr, cp)):
        assert np.array_equal(y[:, pr:pr + cr], y[:, pr + Nr:pr + cr + Nr])   # the prefix is cyclic
        for a, sh, shr in ((0, 1.0, 1.0), (1, shift, shift_r)):
            X = np.fft.fft(x[a, p + c:p + c + N] * sh)
            Y = np.fft.fft(y[a, pr + cr:pr + cr + Nr] * shr)
            kept = np.concatenate([np.arange(Nr // 2), np.arange(N - Nr // 2, N)])
            keptr = np.concatenate([np.arange(Nr // 2), np.arange(Nr - Nr // 2, Nr)])
            worst = max(worst, float(np.abs(Y[keptr] - X[kept]).max() / np.abs(X[kept]).max()))
    assert worst < 1e-9, worst


def test_converter_prach_window():
    for nof_prb in (50, 100):
        N, Nr = SYMBOL_SZ_3GPP[nof_prb], SYMBOL_SZ_SRSRAN[nof_prb]
        rng = np.random.default_rng(nof_prb)
        cp, cpr = 3168 * N // 2048, 3168 * Nr // 2048
        X = np.zeros(12 * N, dtype=np.complex128)
        b = (np.arange(839) - 420 + 200) % (12 * N)     # 839 bins of 1.25 kHz somewhere inside the band
        X[b] = np.exp(2j * np.pi * rng.random(839))
        s = np.fft.ifft(X)
        x = np.zeros(15 * N, dtype=np.complex128)
        x[cp:cp + 12 * N] = s
        x[:cp] = s[12 * N - cp:]
        y = convert_prach_subframe(x, nof_prb, dtype=None)
        Y = np.fft.fft(y[cpr:cpr + 12 * Nr])
        br = (np.arange(839) - 420 + 200) % (12 * Nr)
        assert np.abs(Y[br] - X[b]).max() < 1e-9
        assert np.array_equal(y[:cpr], y[12 * Nr:12 * Nr + cpr])


def test_oracle_1536_transform_error_is_measurable():
    """the yardstick of the 384- / 768-point transform test on the GPU: float32 error of the oracle's 1536-point transform against float64"""
    e = oracle_fft1536_error()
    print("oracle o_fft(1536) vs float64: largest relative RMS error per symbol %.3e" % e)
    assert 1e-8 < e < 1e-6, e   # float32 rounding (6e-8) accumulated over 9 + 1 stages; anything else means the helper is broken


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_compared_streams_stay_away_from_the_last_turbo_iteration(name):
    """the GPU tests demand equal records from soft values that differ in their last bits: that is only sound when no CRC verdict of the oracle hangs on the
    last allowed iteration.  Checked here on the CPU, asserted again where the records are compared."""
    sc, tti0, iq, orecs, otrace, _ = stream(name)
    assert len(orecs) >= 10, len(orecs)
    assert any(c["ok"] for o in otrace for c in o["cbs"])
    assert edge_blocks(otrace) == [] and failed_records(orecs) == []


@pytest.mark.parametrize("nof_prb", [50, 100])
def test_ul_mode_streams_stay_away_from_the_last_turbo_iteration(nof_prb):
    from srs_streams import ul_mode_stream
    sc, tti0, iq, orecs, otrace = ul_mode_stream(nof_prb)
    assert sum(1 for r in orecs if r[1] == 0) >= 10 and sum(1 for r in orecs if r[1] == 1) >= 5   # uplink and downlink records
    assert edge_blocks(otrace) == [] and failed_records(orecs) == []

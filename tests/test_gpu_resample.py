"""The GPU polyphase resampler (k_resample: lsn_resample, lsn_phy_process_file_rate) against the float64 model of tests/resample_model.py, against exact
tones, against itself (one call = the same span in pieces, bit for bit) and end to end: foreign-rate files replayed to the oracle's record stream."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from parity import gpu_records
from resample_cases import CASES, FAR, LEAD, PAIRS, check_tones, foreign_capture
from resample_model import Plan, passband_hz
from srs_streams import edge_blocks, failed_records

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
INVALID = -2   # LSN_ERROR_INVALID_INPUTS


def _phy(sc, batch=8, rates=la.RATES_3GPP, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(rates)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


def _ofdm_like(rng, n, nant, occupied):
    """band-limited noise: random carriers on the occupied fraction of the band, the shape of an LTE downlink at the input rate"""
    X = np.zeros((n, nant), dtype=np.complex128)
    k = int(n * occupied / 2)
    X[:k] = rng.standard_normal((k, nant)) + 1j * rng.standard_normal((k, nant))
    X[n - k:] = rng.standard_normal((k, nant)) + 1j * rng.standard_normal((k, nant))
    x = np.fft.ifft(X, axis=0)
    return x / np.sqrt(np.mean(np.abs(x) ** 2))


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_kernel_against_the_model_within_the_float32_dot_product_bound(rate_in, rate_out, nof_prb, fmt):
    """|y_gpu - y_model| <= (T + 2) 2^-24 sum_j |c_j| |x_j| per output: T fused multiply-adds into one float32 accumulator, one rounding of the bank entry
    and one of the phase interpolation.  The model is handed the float32 samples the kernel forms (integer * scale, one rounding)."""
    rng = np.random.default_rng(int(rate_in) % 1000 + fmt)
    B = passband_hz(nof_prb)
    n_out = 6000
    for nant, kind, first, frac in ((1, "random", 0, 0.0), (2, "ofdm", 12345, 0.625), (2, "random", FAR, 0.3)):
        plan = Plan(rate_in, rate_out, B, first, frac)
        lo, hi = plan.span(0, n_out)
        base = max(lo, 0)
        n_in = hi - base
        if kind == "random":
            x = (rng.standard_normal((n_in, nant)) + 1j * rng.standard_normal((n_in, nant))) / np.sqrt(2)
        else:
            x = _ofdm_like(rng, n_in, nant, 2 * B / rate_in)
        if fmt == la.FILE_CF32:
            raw = x.astype(np.complex64)
            x32, scale = raw, 0.0
        else:
            full, dt, scale = ((32767, np.int16, np.float32(1.0 / 9000.0)), (127, np.int8, np.float32(1.0 / 30.0)))[fmt - 1]   # not powers of two: the product rounds
            raw = np.clip(np.round(np.stack([x.real, x.imag], axis=-1) / float(scale)), -full, full).astype(dt)
            v = raw.astype(np.float32) * scale
            x32 = v[..., 0] + 1j * v[..., 1]
        y = la.resample(raw, rate_in, rate_out, n_out=n_out, first_sample=first, first_frac=frac, in_base=base, passband_hz=B, sample_format=fmt, sample_scale=float(scale))
        ref, bound = plan.apply(x32, 0, n_out, in_base=base, with_bound=True)
        assert y.shape == (nant, n_out)
        err = np.abs(y.T.astype(np.complex128) - ref)
        lim = (plan.taps + 2) * 2.0 ** -24 * bound
        worst = float(np.max(err / np.maximum(lim, 1e-300)))
        print("resample %.6f -> %.2f fmt %d %s x%d: T = %d, largest error / bound = %.3f" % (rate_in / 1e6, rate_out / 1e6, fmt, kind, nant, plan.taps, worst))
        assert np.all(err <= lim), worst
        assert la.resample_span(n_out, 0, rate_in, rate_out, first, frac, passband_hz=B)["taps"] == plan.taps


def _gpu(passband, plan, x, in_base, n_out):
    first, frac = plan.start >> 64, (plan.start & (2 ** 64 - 1)) / 2.0 ** 64
    return la.resample(x.astype(np.complex64), plan.rate_in, plan.rate_out, n_out=n_out, first_sample=first, first_frac=frac, in_base=in_base,
                       passband_hz=passband)[0].astype(np.complex128)


@pytest.mark.parametrize("first_sample", [0, FAR])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_kernel_meets_the_quality_requirement_on_exact_tones(rate_in, rate_out, nof_prb, first_sample):
    worst_pass, worst_land = check_tones(functools.partial(_gpu, passband_hz(nof_prb)), rate_in, rate_out, nof_prb, first_sample=first_sample, first_frac=0.25)   # 0.25: exact in 64.64 and in a double
    print("resample GPU %.6f -> %.2f MS/s, %d PRB, first_sample %d: pass band %.1f dB, landing in band %.1f dB" %
          (rate_in / 1e6, rate_out / 1e6, nof_prb, first_sample, 20 * np.log10(worst_pass), 20 * np.log10(max(worst_land, 1e-30))))
    assert worst_pass <= 1e-3 and worst_land <= 1e-3, (worst_pass, worst_land)


@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_one_call_and_the_same_span_in_pieces_are_bit_identical(rate_in, rate_out, nof_prb):
    rng = np.random.default_rng(7)
    B, n_out, first, frac = passband_hz(nof_prb), 20000, 5000, 0.4375
    plan = Plan(rate_in, rate_out, B, first, frac)
    lo, hi = plan.span(0, n_out)
    x = (rng.standard_normal((hi - lo, 2)) + 1j * rng.standard_normal((hi - lo, 2))).astype(np.complex64)
    kw = dict(first_sample=first, first_frac=frac, passband_hz=B)
    whole = la.resample(x, rate_in, rate_out, n_out=n_out, in_base=lo, **kw)
    parts = []
    for a, b in ((0, 1), (1, 2), (2, 513), (513, 7777), (7777, 16384), (16384, 20000)):
        plo, phi = plan.span(a, b - a)    # each piece is handed only the input it reads
        parts.append(la.resample(x[plo - lo:phi - lo], rate_in, rate_out, n_out=b - a, in_base=plo, out_first=a, **kw))
    parts = np.concatenate(parts, axis=1)
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))


def _write(td, f, fmt):
    """file samples [sample][antenna] complex128 -> path, sample_scale"""
    if fmt == la.FILE_CF32:
        p = os.path.join(td, "c.cf32")
        f.astype(np.complex64).tofile(p)
        return p, 0.0
    scale = 2.0 ** -13   # as test_gpu_srs_rates: quantisation noise 80 dB under the signal
    assert float(np.abs(f.real).max()) < 3.9 and float(np.abs(f.imag).max()) < 3.9
    p = os.path.join(td, "c.sc16")
    np.round(np.stack([f.real, f.imag], axis=-1) / scale).astype(np.int16).tofile(p)
    return p, scale


def _replay(sc, opt, path, fmt, scale, rate_in, tti0, rates=la.RATES_3GPP, offset=LEAD, frac=0.0, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        phy = _phy(sc, rates=rates, **opt)
        n = phy.process_file(path, start_tti=tti0, offset_time=offset, sample_format=fmt, sample_scale=scale, sample_rate=rate_in, offset_time_frac=frac)
        g = gpu_records(phy)
        phy.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return n, g


@pytest.mark.parametrize("case", sorted(CASES))
def test_foreign_rate_files_replay_to_the_oracle_records(case):
    """every stream and rate pair of the CPU round trip, as a cf32 and an sc16 file, with both LSN_FILE_MMAP settings and two LSN_FILE_BLOCK sizes (5 does
    not divide 12, 20 or 48 subframes); the 25 MS/s file of the 100-PRB stream in both sampling modes of the Phy (-> 30.72 and -> 23.04 MS/s)"""
    sc, tti0, orecs, otrace, opt, rate_in, native, f = foreign_capture(case)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    nsf = int(round((len(f) - 2 * LEAD) * native / rate_in / (native / 1000)))
    modes = [la.RATES_3GPP] + ([la.RATES_SRSRAN] if case == "prb100_from_25" else [])
    with tempfile.TemporaryDirectory() as td:
        for fmt in (la.FILE_CF32, la.FILE_SC16):
            path, scale = _write(td, f, fmt)
            for rates in modes:
                for env in ({"LSN_FILE_MMAP": "0", "LSN_FILE_BLOCK": "5"}, {"LSN_FILE_MMAP": "1", "LSN_FILE_BLOCK": "5"}, {"LSN_FILE_MMAP": "0", "LSN_FILE_BLOCK": "800"},
                            {"LSN_FILE_MMAP": "1", "LSN_FILE_BLOCK": "16"}):
                    n, g = _replay(sc, opt, path, fmt, scale, rate_in, tti0, rates=rates, env=env)
                    assert n == nsf, (n, nsf, fmt, rates, env)
                    assert g == orecs, "fmt %d mode %d %s: %d records vs %d" % (fmt, rates, env, len(g), len(orecs))
        if "ppm" in case:
            # the same file replayed as if its clock were exact: 48 subframes x 7680 x 150e-6 = 55 samples of drift against a cyclic prefix of 36
            path, scale = _write(td, f, la.FILE_CF32)
            n, g = _replay(sc, opt, path, la.FILE_CF32, scale, 7.68e6, tti0)
            assert n >= 40 and len(g) < len(orecs) and g != orecs, (n, len(g), len(orecs))


def test_chain_head_resampled_cell_search_mib_and_replay():
    """a 25 MS/s recording of a 20 MHz cell that starts at an unknown, fractional instant: the head resampled by lsn_resample, cell search on it, sf_start
    scaled by rate_in / rate_out as the offset (integer part and fraction), LSN_TTI_FROM_MIB replay -> the oracle's records of the subframes replayed"""
    from lsn_testlib import scenario
    from parity import gen_subframes, oracle_records, run_oracle
    from resample_cases import fft_convert
    sc = scenario("cfg2", seed=9, start_tti=10 * 300 + 2, nof_prb=100, nof_rx=1, cell_id=401, n_rnti=8, dl_min=2, dl_max=3, snr_db=30.0)
    rate_in, rate_out, B = 25e6, 30.72e6, passband_hz(100)
    tti0, iq, _ = gen_subframes(sc, 30)
    y = fft_convert(iq[:, 0].reshape(-1), 625, 768)
    # unknown start: the recording begins 4321.37 samples (of ITS rate) before the stream: shift by the fraction with a phase ramp (exact for the periodic
    # capture), then by the whole samples with receiver noise in front
    Y = np.fft.fft(y)
    y = np.fft.ifft(Y * np.exp(-2j * np.pi * np.fft.fftfreq(len(y)) * 0.37))
    rng = np.random.default_rng(3)
    lead = 4321
    cap = np.concatenate([0.02 * (rng.standard_normal(lead) + 1j * rng.standard_normal(lead)), y, y[:2000]]).astype(np.complex64)
    true_start = lead + 0.37                                        # input position of the stream's first sample
    head = la.resample(cap[:int(0.02 * rate_in)], rate_in, rate_out, passband_hz=B)[0]     # 20 ms
    rc, s = la.cell_search(head, 100, nof_periods=1)
    assert rc == 1 and s.cell_id == 401 and s.cp == 0
    k = (s.sf_idx - tti0) % 5
    start = int(s.sf_start) * rate_in / rate_out                    # in samples of the file
    assert abs(start - (true_start + k * 25000)) <= 1.0, (start, true_start, k)
    first0 = k + ((10 - s.sf_idx) % 10)                             # the stream's subframe that is subframe 0 of the next radio frame
    start += (first0 - k) * 25000.0
    _, _, orecs = run_oracle(sc, tti0 + first0, iq[first0:], taps=False)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "capture.cf32")
        cap.tofile(path)
        phy = _phy(sc)
        n = phy.process_file(path, start_tti=la.TTI_FROM_MIB, offset_time=int(start), offset_time_frac=start - int(start), sample_rate=rate_in)
        g, o = gpu_records(phy), oracle_records(orecs)
        phy.close()
    assert n == 30 - first0
    assert len(o) > 10 and g == o, (len(g), len(o))


def test_refusals_decode_nothing_and_leave_the_phy_usable():
    sc, tti0, orecs, otrace, opt, rate_in, native, f = foreign_capture("prb100_from_25")
    L = la.lib()
    with tempfile.TemporaryDirectory() as td:
        path, _ = _write(td, f, la.FILE_CF32)
        import srs_streams as S
        _, _, iq, _, _, _ = S.stream(CASES["prb100_from_25"][0])
        pn = os.path.join(td, "native.cf32")
        np.ascontiguousarray(iq.transpose(0, 2, 1)).tofile(pn)
        phy = _phy(sc, **opt)
        fc = la.FileCfg(sc["nof_rx"], LEAD, 0.0, la.FILE_CF32, 0.0)
        done = C.c_uint64(99)
        size = C.sizeof(la.FileRate)
        for fr in (la.FileRate(size, 0, 18e6, 0.0),              # below 2 x the occupied half-band: the rate cannot carry the cell
                   la.FileRate(size, 0, 4.0001 * 30.72e6, 0.0),  # above 4 x the output rate
                   la.FileRate(size + 8, 0, 25e6, 0.0), la.FileRate(0, 0, 25e6, 0.0),   # a struct_size the library does not know
                   la.FileRate(size, 0, 0.0, 0.0), la.FileRate(size, 0, -25e6, 0.0), la.FileRate(size, 0, float("nan"), 0.0), la.FileRate(size, 0, 25e6, -0.5)):
            assert L.lsn_phy_process_file_rate(phy._h, os.fsencode(path), C.byref(fc), C.byref(fr), tti0, 0, 0, C.byref(done)) == INVALID
            assert done.value == 0 and gpu_records(phy) == []
        out = np.zeros(100, dtype=np.complex64)
        x = np.zeros(1000, dtype=np.complex64)
        good = la._resample_cfg(1, 25e6, 30.72e6, 0, 0.0, 0, 0, passband_hz(100), la.FILE_CF32, 0.0)
        assert L.lsn_resample(0, x.ctypes.data, 0, 1000, C.byref(good), out.ctypes.data, 0, 100) == 0
        for rin, rout, size_, nin in ((18e6, 30.72e6, None, 1000), (123e6, 30.72e6, None, 1000), (25e6, 30.72e6, 48, 1000), (0.0, 30.72e6, None, 1000),
                                      (25e6, 0.0, None, 1000), (25e6, 30.72e6, None, 50)):   # the last: the input does not hold what 100 outputs read
            cfg = la._resample_cfg(1, rin, rout, 0, 0.0, 0, 0, passband_hz(100), la.FILE_CF32, 0.0)
            if size_ is not None:
                cfg.struct_size = size_
            assert L.lsn_resample(0, x.ctypes.data, 0, nin, C.byref(cfg), out.ctypes.data, 0, 100) == INVALID
        # the old entry point on the same Phy: the native-rate file with the old result
        assert phy.process_file(pn, start_tti=tti0) == iq.shape[0]
        assert gpu_records(phy) == orecs
        phy.close()

"""The channel filter in front of the GPU resampler (k_chan_fir; lsn_channel_filter, lsn_phy_set_channel_filter, stopband_hz of process_file_cells) against the
float64 model of tests/chanfilt_model.py, against exact tones, against itself (pieces), and end to end: the recordings whose neighbour carrier is 20 dB stronger
than the wanted cell - which the resampler alone does not decode completely - replayed to the oracle's records, one cell per call and both in one pass."""
import contextlib
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from chanfilt_cases import B100, GEOMETRIES, NSF, RATE, STOP, TONE_CASES, check_filter_tones, quantise, recording
from chanfilt_model import Design
from ddc_cases import recording as ddc_recording
from parity import gpu_records
from resample_cases import FAR, LEAD, Q
from srs_streams import edge_blocks, failed_records

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
TILE = 1024
KERNEL_GEOMETRIES = [GEOMETRIES[3], GEOMETRIES[0], GEOMETRIES[1], (RATE, B100, B100 + 0.0049 * RATE, 512)]   # L = 8, 88, 498, 512


def _phy(sc, batch=8, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(la.RATES_3GPP)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


@contextlib.contextmanager
def _block(n):
    old = os.environ.get("LSN_FILE_BLOCK")
    os.environ["LSN_FILE_BLOCK"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LSN_FILE_BLOCK", None)
        else:
            os.environ["LSN_FILE_BLOCK"] = old


def _samples(rng, n, nant, fmt):
    """-> (array to hand to the library, sample_scale, the float32 values the product forms from it as complex64 [n][nant])"""
    x = (rng.standard_normal((n, nant)) + 1j * rng.standard_normal((n, nant))) / np.sqrt(2)
    if fmt == la.FILE_CF32:
        raw = x.astype(np.complex64)
        return raw, 0.0, raw
    full, dt, scale = ((32767, np.int16, np.float32(1.0 / 9000.0)), (127, np.int8, np.float32(1.0 / 30.0)))[fmt - 1]   # not powers of two: the product rounds
    raw = np.clip(np.round(np.stack([x.real, x.imag], axis=-1) / float(scale)), -full, full).astype(dt)
    v = raw.astype(np.float32) * scale
    return raw, float(scale), v[..., 0] + 1j * v[..., 1]


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
@pytest.mark.parametrize("rate,B,S,L", KERNEL_GEOMETRIES)
def test_kernel_against_the_model_within_the_dot_product_and_nco_bound(rate, B, S, L, fmt):
    """|y_gpu - y_model| <= ((2L + 3) 2^-24 + 2^-18) sum |g| |x| per output: (2L + 3) 2^-24 is the float32 dot product of 2L + 1 terms (the bound of
    test_gpu_resample.py for T terms, (T + 2) 2^-24), 2^-18 the mixer's.  Tile sizes around the kernel's 1024, out_first off the tile grid, the
    outputs that read the zeros in front of sample 0, and a base ten minutes into the recording."""
    rng = np.random.default_rng(L + fmt + 70)
    m = Design(rate, B, S)
    assert m.L == L
    n_in = 6000
    for nant, base, offsets in ((1, 0, (0.0, 9.9e6)), (2, FAR, (-9.9e6,))):
        raw, scale, x32 = _samples(rng, n_in, nant, fmt)
        for f0 in offsets:
            for out_first, n_out in ((0, 3 * TILE + 7), (777, TILE - 1), (777, TILE), (333, TILE + 1), (1501, 3 * TILE + 7)):
                if base:
                    out_first += base + L               # (base 0, out_first 0: the first L outputs read in front of the recording)
                if out_first + n_out + L > base + n_in:
                    n_out = base + n_in - L - out_first
                y = la.channel_filter(raw, rate, B, S, n_out=n_out, center_offset_hz=f0, in_base=base, out_first=out_first, sample_format=fmt, sample_scale=scale)
                ref, bound = m.apply(x32, base, out_first, n_out, f0, with_bound=True)
                assert y.shape == (n_out, nant)
                err = np.abs(y.astype(np.complex128) - ref)
                lim = ((2 * L + 3) * 2.0 ** -24 + 2.0 ** -18) * bound
                worst = float(np.max(err / np.maximum(lim, 1e-300)))
                print("chan fir L %d fmt %d x%d offset %+.1f kHz base %d out_first %d n_out %d: largest error / bound = %.3f" %
                      (L, fmt, nant, f0 / 1e3, base, out_first, n_out, worst))
                assert np.all(err <= lim), worst
                assert float(np.sqrt(np.mean(np.abs(ref) ** 2))) > 0.05    # (the comparison is not one of zeros)


@pytest.mark.parametrize("base", [0, FAR])
@pytest.mark.parametrize("f0", [0.0, -9.9e6 * 0.77])
def test_one_call_and_the_same_span_in_pieces_are_bit_identical(f0, base):
    """y1[n] is a function of (input, configuration, n): pieces cut off the tile grid, each handed only the input it reads, give the bits of one call"""
    rng = np.random.default_rng(11)
    for rate, B, S, L in (GEOMETRIES[0], GEOMETRIES[1]):
        n_out, first = 5000, base + (L if base else 0) + 333
        lo, hi = max(first - L, 0), first + n_out + L
        x = (rng.standard_normal((hi - lo, 2)) + 1j * rng.standard_normal((hi - lo, 2))).astype(np.complex64)
        kw = dict(center_offset_hz=f0)
        whole = la.channel_filter(x, rate, B, S, n_out=n_out, in_base=lo, out_first=first, **kw)
        parts = []
        for a, b in ((0, 1), (1, 2), (2, 1023), (1023, 1030), (1030, 3333), (3333, 5000)):
            plo, phi = max(first + a - L, 0), first + b + L
            parts.append(la.channel_filter(x[plo - lo:phi - lo], rate, B, S, n_out=b - a, in_base=plo, out_first=first + a, **kw))
        parts = np.concatenate(parts, axis=0)
        assert float(np.abs(whole).max()) > 0 and np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
        other = la.channel_filter(x, rate, B, S, n_out=n_out, in_base=lo, out_first=first, center_offset_hz=f0 + 1e6)
        assert not np.array_equal(whole.view(np.uint32), other.view(np.uint32))


@pytest.mark.parametrize("base", [0, FAR])
@pytest.mark.parametrize("geometry,k0s", TONE_CASES)
def test_kernel_meets_the_selectivity_requirement(geometry, k0s, base):
    """the requirement of test_chanfilt_model.py on the kernel: |f| <= B within -60 dB relative RMS, |f| >= S at least 77 dB down"""
    rate, B, S, L = geometry
    m = Design(rate, B, S)
    for k0 in k0s:
        f0 = rate * k0 / Q

        def fn(x, in_base, n0, n):
            return la.channel_filter(x.astype(np.complex64), rate, B, S, n_out=n, center_offset_hz=f0, in_base=in_base, out_first=n0)[:, 0].astype(np.complex128)
        worst_pass, worst_stop = check_filter_tones(fn, m, k0, base)
        print("chan fir GPU L = %d, offset %+.1f kHz, base %d: pass band %.1f dB, stop band %.1f dB" %
              (L, f0 / 1e3, base, 20 * np.log10(worst_pass), 20 * np.log10(worst_stop)))
        assert worst_pass <= 1e-3 and worst_stop <= 10 ** (-77 / 20), (k0, worst_pass, worst_stop)


def _write(td, f, fmt, name="c"):
    raw, scale, _ = quantise(f, fmt)
    p = os.path.join(td, name + (".cf32", ".sc16")[fmt])
    raw.tofile(p)
    return p, scale


def _replay(sc, opt, path, fmt, scale, rate_in, f0, tti0, stop, offset=LEAD, **kw):
    phy = _phy(sc, **opt)
    try:
        assert phy.set_channel_filter(stop)
        n = phy.process_file_rate(path, rate_in, center_offset_hz=f0, start_tti=tti0, offset_time=offset, sample_format=fmt, sample_scale=scale, **kw)
        return n, gpu_records(phy)
    finally:
        phy.close()


@pytest.mark.parametrize("case,fmt", [("b_wanted", la.FILE_CF32), ("a_wanted", la.FILE_CF32), ("b_wanted", la.FILE_SC16)])
def test_a_cell_next_to_a_carrier_20_dB_stronger_replays_to_the_oracle_records(case, fmt):
    """the round-trip cases of test_chanfilt_model.py through set_channel_filter(SPACING - B) + process_file_rate, at two block sizes: the oracle's records, byte
    for byte.  The same file without the filter does not return them (this is the hole DESIGN 3.1b documented)."""
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording(case)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, f, fmt)
        for blk in (5, 800):                    # 5 divides neither 12 subframes nor the shrunk block
            with _block(blk):
                n, g = _replay(sc, opt, path, fmt, scale, rate_in, f0, tti0, STOP)
            assert n == NSF, (n, blk)
            assert g == orecs, "block %d: %d records vs %d" % (blk, len(g), len(orecs))
        with _block(5):
            n, g = _replay(sc, opt, path, fmt, scale, rate_in, f0, tti0, 0.0)
        print("%s fmt %d without the filter: %d records, the oracle has %d" % (case, fmt, len(g), len(orecs)))
        assert n == NSF and g != orecs


def test_tti_from_mib_resamples_through_both_stages():
    from ddc_cases import cell
    from parity import oracle_records, run_oracle
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording("b_wanted")
    _, _, iq, _, _, _ = cell("B")
    first0 = (10 - tti0 % 10) % 10                      # the stream's subframe that is subframe 0 of a radio frame
    _, _, want = run_oracle(sc, tti0 + first0, iq[first0:], taps=False, **opt)
    want = oracle_records(want)
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, f, la.FILE_CF32)
        with _block(5):
            n, g = _replay(sc, opt, path, la.FILE_CF32, scale, rate_in, f0, la.TTI_FROM_MIB, STOP, offset=LEAD + first0 * 61440)
    assert n == NSF - first0
    assert len(want) > 10 and g == want, (len(g), len(want))


def test_a_file_at_the_engines_rate_goes_through_both_stages_when_the_filter_is_set():
    """a 25-PRB capture at its own 7.68 MS/s, no offset, no fraction: with the filter set neither process_file nor process_file_rate takes the k_file_unpack
    shortcut - a stop band the filter cannot meet is refused (35 kHz behind the pass band: L > 512), one it can meet (L = 16) replays to the oracle's records"""
    from ddc_cases import cell
    sc, tti0, iq, orecs, _, opt = cell("prb25_2port")
    B = 15000.0 * (6 * 25 + 1)
    with tempfile.TemporaryDirectory() as td:
        pn = os.path.join(td, "native.cf32")
        np.ascontiguousarray(iq.transpose(0, 2, 1)).tofile(pn)
        phy = _phy(sc, **opt)
        try:
            assert la.channel_filter_design(7.68e6, B, 3.5e6)["L"] == 16
            assert phy.set_channel_filter(B + 35e3)
            for call in (lambda: phy.process_file(pn, start_tti=tti0), lambda: phy.process_file_rate(pn, 7.68e6, start_tti=tti0)):
                with pytest.raises(RuntimeError):
                    call()
                assert gpu_records(phy) == []
            assert phy.set_channel_filter(3.5e6)
            # the last 16 + T / 2 samples of the file are not followed by what the two filters read: the last subframe is not produced
            assert phy.process_file(pn, start_tti=tti0) == iq.shape[0] - 1
            g = gpu_records(phy)
        finally:
            phy.close()
        phy = _phy(sc, **opt)
        try:
            assert phy.process_file(pn, start_tti=tti0, max_subframes=iq.shape[0] - 1) == iq.shape[0] - 1
            plain = gpu_records(phy)
        finally:
            phy.close()
    assert len(plain) >= 10 and g == plain, (len(g), len(plain))


def test_both_cells_of_the_recording_in_one_pass():
    """process_file_cells with stopband_hz from cells_stopbands: the weak cell's records are the oracle's and its own filtered single-cell replay's; so are the
    strong cell's"""
    b = recording("b_wanted")                            # B at amplitude 1, A at amplitude 10: one recording, two cells
    a = recording("a_wanted")
    sc_a, tti_a, orecs_a, opt_a = a[0], a[1], a[2], a[4]
    sc_b, tti_b, orecs_b, opt_b = b[0], b[1], b[2], b[4]
    stops = la.cells_stopbands([-9.9e6, 9.9e6], [100, 100], RATE)
    assert stops == [STOP, STOP]
    cells = [(sc_b, opt_b, dict(center_offset_hz=-9.9e6, start_tti=tti_b, offset_time=LEAD, stopband_hz=stops[0]), orecs_b),
             (sc_a, opt_a, dict(center_offset_hz=9.9e6, start_tti=tti_a, offset_time=LEAD, stopband_hz=stops[1]), orecs_a)]
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, b[-1], la.FILE_CF32)
        for blk in (5, 16):
            with _block(blk):
                phys = [_phy(sc, **opt) for sc, opt, _, _ in cells]
                try:
                    done = la.process_file_cells(path, RATE, [(p, kw) for p, (_, _, kw, _) in zip(phys, cells)])
                    got = [gpu_records(p) for p in phys]
                finally:
                    for p in phys:
                        p.close()
                assert done == [NSF, NSF], done
                for (sc, opt, kw, orecs), g in zip(cells, got):
                    n, single = _replay(sc, opt, path, la.FILE_CF32, scale, RATE, kw["center_offset_hz"], kw["start_tti"], kw["stopband_hz"])
                    assert n == NSF and g == single, "cell %d block %d: one pass %d records, single %d" % (sc["cell_id"], blk, len(g), len(single))
                    assert g == orecs, "cell %d block %d: %d records vs %d" % (sc["cell_id"], blk, len(g), len(orecs))


def test_zero_switches_the_filter_off_mixes_are_refused_and_a_refused_stopband_leaves_the_phy_usable():
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = ddc_recording("two_cells_a")
    other = ddc_recording("two_cells_b")
    with tempfile.TemporaryDirectory() as td:
        path, scale = _write(td, f, la.FILE_CF32)
        with _block(5):
            phy = _phy(sc, **opt)
            pb = _phy(other[0], **other[4])
            try:
                for bad in (-1.0, float("nan"), float("inf")):
                    assert not phy.set_channel_filter(bad)
                # a stop band the filter cannot meet (100 kHz behind the pass band: L > 512) and one behind rate / 2: refused when the replay starts, nothing decoded
                for bad in (B100 + 100e3, B100, 1.0, RATE / 2 + 1.0):
                    assert phy.set_channel_filter(bad)
                    with pytest.raises(RuntimeError):
                        phy.process_file_rate(path, rate_in, center_offset_hz=f0, start_tti=tti0, offset_time=LEAD)
                    assert gpu_records(phy) == []
                # a filtered / unfiltered mix of cells
                assert phy.set_channel_filter(STOP) and pb.set_channel_filter(0.0)
                ka = dict(center_offset_hz=f0, start_tti=tti0, offset_time=LEAD)
                kb = dict(center_offset_hz=other[7], start_tti=other[1], offset_time=LEAD)
                with pytest.raises(ValueError):
                    la.process_file_cells(path, rate_in, [(phy, ka), (pb, kb)])
                with pytest.raises(ValueError):
                    la.process_file_cells(path, rate_in, [(phy, dict(ka, stopband_hz=0.0)), (pb, dict(kb, stopband_hz=STOP))])
                assert gpu_records(phy) == [] and gpu_records(pb) == []
                # the plan of the filtered pass reads L = 88 more samples on both sides than the unfiltered one
                assert pb.set_channel_filter(0.0) and phy.set_channel_filter(0.0)
                plain = la.file_cells_span(rate_in, [(phy, ka), (pb, kb)], len(f), block=1, blk_subframes=5, nof_antennas=2)
                assert phy.set_channel_filter(STOP) and pb.set_channel_filter(STOP)
                filt = la.file_cells_span(rate_in, [(phy, ka), (pb, kb)], len(f), block=1, blk_subframes=5, nof_antennas=2)
                assert filt["blk_used"] == plain["blk_used"] and filt["first_subframe"] == plain["first_subframe"]
                assert (filt["in_lo"], filt["in_hi"]) == (plain["in_lo"] - 88, plain["in_hi"] + 88)
                # 0 after a non-zero value: the replay of before, on the same Phy
                assert phy.set_channel_filter(0.0)
                n = phy.process_file_rate(path, rate_in, center_offset_hz=f0, start_tti=tti0, offset_time=LEAD)
                assert n == NSF and gpu_records(phy) == orecs
            finally:
                phy.close()
                pb.close()

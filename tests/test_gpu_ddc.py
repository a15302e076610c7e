"""Frequency translation in front of the GPU resampler (center_offset_hz of lsn_resample and lsn_phy_process_file_rate; the mixing instantiations of
k_resample) against the float64 model of tests/ddc_cases.py, against exact tones off the recording's centre, against itself (pieces, and offset 0 against the
old struct) and end to end: recordings that hold a cell off their centre - two cells in one 61.44 MS/s file among them - replayed to the oracle's records."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from ddc_cases import cell, model_resample, offset_hz, offsets_k0, quantise, recording, shifted
from parity import gpu_records
from resample_cases import FAR, LEAD, PAIRS, check_tones
from resample_model import Plan, passband_hz
from srs_streams import edge_blocks, failed_records

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
INVALID = -2   # LSN_ERROR_INVALID_INPUTS


def _phy(sc, batch=8, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(la.RATES_3GPP)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_kernel_against_the_model_within_the_dot_product_and_nco_bound(rate_in, rate_out, nof_prb, fmt):
    """|y_gpu - y_model| <= ((T + 2) 2^-24 + 2^-18) sum_j |c_j| |x_j| per output.  (T + 2) 2^-24 is the float32 dot product of the plain kernel
    (test_gpu_resample.py).  2^-18 = 3.8e-6 per sample is the mixer's, derived in DESIGN 3.1b: the 42 truncated phase bits turn the sample by at most 2 pi 2^-22 =
    1.5e-6, and the roundings of the two float32 table entries and of the two complex products stay under 0.8e-6.  The model mixes with the exact phase."""
    rng = np.random.default_rng(int(rate_in) % 1000 + fmt + 50)
    B = passband_hz(nof_prb)
    n_out = 6000
    k0s = offsets_k0(rate_in, nof_prb)
    for (nant, first, frac), signs in (((1, 0, 0.0), k0s[:2]), ((2, FAR, 0.3), k0s[2:])):
        plan = Plan(rate_in, rate_out, B, first, frac)
        lo, hi = plan.span(0, n_out)
        base = max(lo, 0)
        n_in = hi - base
        x = (rng.standard_normal((n_in, nant)) + 1j * rng.standard_normal((n_in, nant))) / np.sqrt(2)
        if fmt == la.FILE_CF32:
            raw = x.astype(np.complex64)
            x32, scale = raw, 0.0
        else:
            full, dt, scale = ((32767, np.int16, np.float32(1.0 / 9000.0)), (127, np.int8, np.float32(1.0 / 30.0)))[fmt - 1]   # not powers of two: the product rounds
            raw = np.clip(np.round(np.stack([x.real, x.imag], axis=-1) / float(scale)), -full, full).astype(dt)
            v = raw.astype(np.float32) * scale
            x32 = v[..., 0] + 1j * v[..., 1]
        for k0 in signs:
            f0 = offset_hz(rate_in, k0)
            y = la.resample(raw, rate_in, rate_out, n_out=n_out, first_sample=first, first_frac=frac, in_base=base, passband_hz=B, sample_format=fmt,
                            sample_scale=float(scale), center_offset_hz=f0)
            ref, bound = model_resample(f0, plan, x32, base, n_out, with_bound=True)
            assert y.shape == (nant, n_out)
            err = np.abs(y.T.astype(np.complex128) - ref)
            lim = ((plan.taps + 2) * 2.0 ** -24 + 2.0 ** -18) * bound
            worst = float(np.max(err / np.maximum(lim, 1e-300)))
            print("ddc %.6f -> %.2f fmt %d x%d offset %+.1f kHz first %d: T = %d, largest error / bound = %.3f" %
                  (rate_in / 1e6, rate_out / 1e6, fmt, nant, f0 / 1e3, first, plan.taps, worst))
            assert np.all(err <= lim), worst
            assert float(np.sqrt(np.mean(np.abs(ref) ** 2))) > 0.05    # (the comparison is not one of zeros)


def _gpu(passband, f0, plan, x, in_base, n_out):
    first, frac = plan.start >> 64, (plan.start & (2 ** 64 - 1)) / 2.0 ** 64
    return la.resample(x.astype(np.complex64), plan.rate_in, plan.rate_out, n_out=n_out, first_sample=first, first_frac=frac, in_base=in_base,
                       passband_hz=passband, center_offset_hz=f0)[0].astype(np.complex128)


@pytest.mark.parametrize("first_sample", [0, FAR])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_kernel_meets_the_quality_requirement_on_tones_off_the_centre(rate_in, rate_out, nof_prb, first_sample):
    for k0 in offsets_k0(rate_in, nof_prb):
        f0 = offset_hz(rate_in, k0)
        fn = shifted(functools.partial(_gpu, passband_hz(nof_prb), f0), k0)
        worst_pass, worst_land = check_tones(fn, rate_in, rate_out, nof_prb, first_sample=first_sample, first_frac=0.25)   # 0.25: exact in 64.64 and in a double
        print("ddc GPU %.6f -> %.2f MS/s, %d PRB, offset %+.1f kHz, first_sample %d: pass band %.1f dB, landing in band %.1f dB" %
              (rate_in / 1e6, rate_out / 1e6, nof_prb, f0 / 1e3, first_sample, 20 * np.log10(worst_pass), 20 * np.log10(max(worst_land, 1e-30))))
        assert worst_pass <= 1e-3 and worst_land <= 1e-3, (k0, worst_pass, worst_land)


@pytest.mark.parametrize("first", [5000, FAR])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_one_call_and_the_same_span_in_pieces_are_bit_identical_with_an_offset(rate_in, rate_out, nof_prb, first):
    rng = np.random.default_rng(8)
    B, n_out, frac = passband_hz(nof_prb), 20000, 0.4375
    plan = Plan(rate_in, rate_out, B, first, frac)
    lo, hi = plan.span(0, n_out)
    x = (rng.standard_normal((hi - lo, 2)) + 1j * rng.standard_normal((hi - lo, 2))).astype(np.complex64)
    kw = dict(first_sample=first, first_frac=frac, passband_hz=B, center_offset_hz=-offset_hz(rate_in, offsets_k0(rate_in, nof_prb)[0]) * 0.77)   # not on any grid
    whole = la.resample(x, rate_in, rate_out, n_out=n_out, in_base=lo, **kw)
    parts = []
    for a, b in ((0, 1), (1, 2), (2, 513), (513, 7777), (7777, 16384), (16384, 20000)):
        plo, phi = plan.span(a, b - a)    # each piece is handed only the input it reads
        parts.append(la.resample(x[plo - lo:phi - lo], rate_in, rate_out, n_out=b - a, in_base=plo, out_first=a, **kw))
    parts = np.concatenate(parts, axis=1)
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    plain = la.resample(x, rate_in, rate_out, n_out=n_out, in_base=lo, **dict(kw, center_offset_hz=0.0))
    assert not np.array_equal(whole.view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_offset_zero_in_the_new_struct_equals_the_old_struct_bit_for_bit(fmt):
    rng = np.random.default_rng(9)
    L = la.lib()
    for rate_in, rate_out, nof_prb in PAIRS[:3]:
        B, n_out = passband_hz(nof_prb), 5000
        n_in = la.resample_span(n_out, 0, rate_in, rate_out, 777, 0.5, passband_hz=B)["in_hi"]
        if fmt == la.FILE_CF32:
            x = (rng.standard_normal((n_in, 2)) + 1j * rng.standard_normal((n_in, 2))).astype(np.complex64)
        else:
            x = rng.integers(-120, 120, (n_in, 2, 2)).astype((np.int16, np.int8)[fmt - 1])
        outs = []
        for size, f0 in ((80, 0.0), (72, 0.0), (72, 1e6), (80, -0.0)):     # behind the old size the field is not read
            cfg = la._resample_cfg(2, rate_in, rate_out, 777, 0.5, 0, 0, B, fmt, 0.01, center_offset_hz=f0)
            cfg.struct_size = size
            out = np.zeros((2, n_out), dtype=np.complex64)
            assert L.lsn_resample(0, x.ctypes.data, 0, n_in, C.byref(cfg), out.ctypes.data, 0, n_out) == 0
            outs.append(out)
        assert float(np.abs(outs[0]).max()) > 0
        for o in outs[1:]:
            assert np.array_equal(outs[0].view(np.uint32), o.view(np.uint32))


def _write(td, f, fmt, name="c"):
    raw, scale, _ = quantise(f, fmt)
    p = os.path.join(td, name + (".cf32", ".sc16")[fmt])
    raw.tofile(p)
    return p, scale


def _replay(sc, opt, path, fmt, scale, rate_in, f0, tti0, offset=LEAD, env=None, **kw):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        phy = _phy(sc, **opt)
        n = phy.process_file_rate(path, rate_in, center_offset_hz=f0, start_tti=tti0, offset_time=offset, sample_format=fmt, sample_scale=scale, **kw)
        g = gpu_records(phy)
        phy.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return n, g


ENVS = ({"LSN_FILE_BLOCK": "5"}, {"LSN_FILE_BLOCK": "800"})   # 5 divides neither 12 nor 24 subframes


@pytest.mark.parametrize("case", ["prb50_plus_3p9", "prb25_plus_300k"])
def test_offset_tuned_files_replay_to_the_oracle_records(case):
    """the single-cell cases of the CPU round trip (a 50-PRB cell 3.9 MHz off the centre of a 25 MS/s file; a 25-PRB cell 300 kHz off the centre of a file at its
    own rate: the resampler with equal rates), as a cf32 and an sc16 file, with two block sizes.  Without the offset the file does not decode."""
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording(case)
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    nsf = {50: 20, 25: 24}[sc["nof_prb"]]
    with tempfile.TemporaryDirectory() as td:
        for fmt in (la.FILE_CF32, la.FILE_SC16):
            path, scale = _write(td, f, fmt)
            for env in ENVS:
                n, g = _replay(sc, opt, path, fmt, scale, rate_in, f0, tti0, env=env)
                assert n == nsf, (n, nsf, fmt, env)
                assert g == orecs, "fmt %d %s: %d records vs %d" % (fmt, env, len(g), len(orecs))
        n, g = _replay(sc, opt, path, fmt, scale, rate_in, 0.0, tti0)
        assert n == nsf and g != orecs, (n, len(g), len(orecs))


def test_two_cells_of_one_wideband_file_replay_to_their_oracle_records():
    """one 61.44 MS/s recording, two 100-PRB cells 9.9 MHz either side of its centre at equal power: two Phys on the same file, one per cell, each with its
    cell's offset -> each cell's oracle records.  cf32 and sc16, two block sizes."""
    a = recording("two_cells_a")
    b = recording("two_cells_b")
    assert np.array_equal(a[-1], b[-1]) and a[5] == b[5] == 61.44e6           # the same recording, whichever cell is called the wanted one
    for r in (a, b):
        assert edge_blocks(r[3]) == [] and failed_records(r[2]) == [] and len(r[2]) >= 10
    assert a[2] != b[2] and a[0]["cell_id"] != b[0]["cell_id"]
    with tempfile.TemporaryDirectory() as td:
        for fmt in (la.FILE_CF32, la.FILE_SC16):
            path, scale = _write(td, a[-1], fmt)
            for env in ({"LSN_FILE_BLOCK": "5"}, {"LSN_FILE_BLOCK": "16"}):    # (two Phys hold their block buffers at once: not the 800-subframe default)
                old = os.environ.get("LSN_FILE_BLOCK")
                os.environ.update(env)
                try:
                    phys = [_phy(r[0], **r[4]) for r in (a, b)]                  # both alive at once, on the same file
                    for phy, r in zip(phys, (a, b)):
                        n = phy.process_file_rate(path, r[5], center_offset_hz=r[7], start_tti=r[1], offset_time=LEAD, sample_format=fmt, sample_scale=scale)
                        assert n == 12, (n, fmt, env)
                    for phy, r in zip(phys, (a, b)):
                        g = gpu_records(phy)
                        assert g == r[2], "cell %d fmt %d %s: %d records vs %d" % (r[0]["cell_id"], fmt, env, len(g), len(r[2]))
                        phy.close()
                finally:
                    if old is None:
                        os.environ.pop("LSN_FILE_BLOCK", None)
                    else:
                        os.environ["LSN_FILE_BLOCK"] = old


@pytest.mark.parametrize("case", ["two_cells_a", "two_cells_b"])
def test_chain_head_translated_cell_search_mib_and_replay(case):
    """the two-cell recording: its head translated and resampled by lsn_resample with one cell's offset, cell search on it finds THAT cell (the other one is
    9.9 MHz further away and in the filter's stop and transition bands), sf_start scaled by rate_in / rate_out as the offset, then the LSN_TTI_FROM_MIB replay with
    the same center_offset_hz gives the oracle's records of the subframes replayed"""
    from parity import oracle_records, run_oracle
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording(case)
    _, _, iq, _, _, _ = cell("A" if case == "two_cells_a" else "B")
    cap = f.astype(np.complex64)
    head = la.resample(cap, rate_in, native, passband_hz=passband_hz(100), center_offset_hz=f0)     # all 12 ms: [antenna][n]
    rc, s = la.cell_search(head[0], 100, nof_periods=1)
    assert rc == 1 and s.cell_id == sc["cell_id"] and s.cp == 0, (rc, s.cell_id, sc["cell_id"])
    k = (s.sf_idx - tti0) % 5
    start = int(s.sf_start) * rate_in / native                      # in samples of the file
    assert abs(start - (LEAD + k * 61440)) <= 1.0, (start, k)
    first0 = k + ((10 - s.sf_idx) % 10)                             # the stream's subframe that is subframe 0 of a radio frame
    assert first0 < 10
    start += (first0 - k) * 61440.0
    _, _, want = run_oracle(sc, tti0 + first0, iq[first0:], taps=False, **opt)
    want = oracle_records(want)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "capture.cf32")
        cap.tofile(path)
        phy = _phy(sc, **opt)
        n = phy.process_file_rate(path, rate_in, center_offset_hz=f0, start_tti=la.TTI_FROM_MIB, offset_time=int(start), offset_time_frac=start - int(start))
        g = gpu_records(phy)
        phy.close()
    assert n == 12 - first0
    assert len(want) > 10 and g == want, (len(g), len(want))
    if first0 == 0:
        assert want == orecs


def test_refusals_decode_nothing_and_leave_the_phy_usable():
    sc, tti0, orecs, otrace, opt, rate_in, native, f0, f = recording("prb50_plus_3p9")
    _, _, iq, norecs, _, _ = cell("prb50_1port_extcp")
    L = la.lib()
    with tempfile.TemporaryDirectory() as td:
        path, _ = _write(td, f, la.FILE_CF32)
        pn = os.path.join(td, "native.cf32")
        np.ascontiguousarray(iq.transpose(0, 2, 1)).tofile(pn)
        phy = _phy(sc, **opt)
        fc = la.FileCfg(sc["nof_rx"], LEAD, 0.0, la.FILE_CF32, 0.0)
        done = C.c_uint64(99)
        B = passband_hz(50)
        edge = rate_in / 2 - B
        for fr in (la.FileRate(32, 0, rate_in, 0.0, edge + 1.0), la.FileRate(32, 0, rate_in, 0.0, -edge - 1.0),     # the cell does not lie inside the recording
                   la.FileRate(32, 0, rate_in, 0.0, float("nan")), la.FileRate(32, 0, rate_in, 0.0, float("inf")), la.FileRate(32, 0, rate_in, 0.0, float("-inf")),
                   la.FileRate(40, 0, rate_in, 0.0, f0), la.FileRate(28, 0, rate_in, 0.0, f0), la.FileRate(0, 0, rate_in, 0.0, f0),   # a struct_size the library does not know
                   la.FileRate(32, 0, native, 0.0, native / 2 - B + 1.0)):                                        # equal rates do not excuse the offset from the rule
            assert L.lsn_phy_process_file_rate(phy._h, os.fsencode(path), C.byref(fc), C.byref(fr), tti0, 0, 0, C.byref(done)) == INVALID
            assert done.value == 0 and gpu_records(phy) == []
        out = np.zeros(100, dtype=np.complex64)
        x = np.zeros(1000, dtype=np.complex64)
        good = la._resample_cfg(1, rate_in, native, 0, 0.0, 0, 0, B, la.FILE_CF32, 0.0, center_offset_hz=f0)
        assert L.lsn_resample(0, x.ctypes.data, 0, 1000, C.byref(good), out.ctypes.data, 0, 100) == 0
        for bad in (edge + 1.0, -edge - 1.0, float("nan"), float("inf")):
            cfg = la._resample_cfg(1, rate_in, native, 0, 0.0, 0, 0, B, la.FILE_CF32, 0.0, center_offset_hz=bad)
            assert L.lsn_resample(0, x.ctypes.data, 0, 1000, C.byref(cfg), out.ctypes.data, 0, 100) == INVALID
        with pytest.raises(ValueError):
            phy.process_file(pn, start_tti=tti0, center_offset_hz=1e6)          # no sample_rate: nothing would translate
        # the old entry point on the same Phy: the native-rate file with the old result
        assert phy.process_file(pn, start_tti=tti0) == iq.shape[0]
        assert gpu_records(phy) == norecs
        phy.close()
        # the old struct_size: center_offset_hz is not read, the file is replayed as if the cell sat at its centre
        phy = _phy(sc, **opt)
        old = la.FileRate(24, 0, rate_in, 0.0, f0)
        assert L.lsn_phy_process_file_rate(phy._h, os.fsencode(path), C.byref(fc), C.byref(old), tti0, 0, 0, C.byref(done)) == 0 and done.value == 20
        assert gpu_records(phy) != orecs
        phy.close()

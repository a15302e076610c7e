"""The resampler's wide-ratio run (k_resample_wide, k_resample_cells_wide, k_resample_ring_wide) on the GPU: against the float64 model of
tests/wide_resample_model.py within the float32 dot-product bound, against exact tones, against itself bit for bit (pieces, cells of both geometries in one call,
the ring wrapped anywhere in a run's staged span), and end to end - the 61.44 MS/s recording with a 100-PRB and a 25-PRB cell (ratio 8) replayed to the oracle's
records through the file pass, the single-cell replay, the stream (pushed whole, in irregular pieces, through the smallest ring, tracked, filtered) and the chain
from the carrier scan.  Every record case passed its CPU round trip in test_wide_resample_model.py.

Output rates below 3.84 MS/s stay refused above ratio 4, so no 6-PRB pair is here: ratios 16 and 32 are a 15-PRB cell's pairs."""
import contextlib
import ctypes as C
import functools
import itertools
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
import resample_cases
from ddc_cases import model_resample, quantise
from parity import gpu_records
from resample_cases import FAR, LEAD, check_tones
from resample_model import passband_hz
from wide_resample_model import WIDE_NSF, WIDE_RATE, WidePlan, wide_recording

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
INVALID = -2   # LSN_ERROR_INVALID_INPUTS
# (rate_in, rate_out, nof_prb): just above ratio 4, 8, 10.67, 16, 32 - 8, 8, 16, 16 and 32 lanes per output
PAIRS = [(30.75e6, 7.68e6, 25), (61.44e6, 7.68e6, 25), (61.44e6, 5.76e6, 25), (61.44e6, 3.84e6, 15), (122.88e6, 3.84e6, 15)]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _samples(rng, n, nant, fmt):
    """-> (what the call is handed, sample_scale, the float32 values the kernel forms)"""
    x = (rng.standard_normal((n, nant)) + 1j * rng.standard_normal((n, nant))) / np.sqrt(2)
    if fmt == la.FILE_CF32:
        raw = x.astype(np.complex64)
        return raw, 0.0, raw
    full, dt, scale = ((32767, np.int16, np.float32(1.0 / 9000.0)), (127, np.int8, np.float32(1.0 / 30.0)))[fmt - 1]   # not powers of two: the product rounds
    raw = np.clip(np.round(np.stack([x.real, x.imag], axis=-1) / float(scale)), -full, full).astype(dt)
    v = raw.astype(np.float32) * scale
    return raw, float(scale), v[..., 0] + 1j * v[..., 1]


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_kernel_against_the_model_within_the_float32_dot_product_bound(rate_in, rate_out, nof_prb, fmt):
    """|y_gpu - y_model| <= ((T + 2) 2^-24 + [mixing] 2^-18) sum_j |c_j| |x_j| per output.  The dot-product bound holds for any order of summation, so the G
    partial sums and their butterfly are covered by the bound of the one-accumulator kernel; 2^-18 is the NCO's (test_gpu_ddc.py)"""
    rng = np.random.default_rng(int(rate_in) % 1000 + 7 * fmt)
    B, n_out = passband_hz(nof_prb), 3000
    f0 = round(0.25 * rate_in / 1e3) * 1e3
    for nant, first, frac, off in ((1, 0, 0.0, 0.0), (2, 0, 0.625, f0), (1, FAR, 0.3, -f0), (2, FAR, 0.0, 0.0)):
        plan = WidePlan(rate_in, rate_out, B, first, frac)
        lo, hi = plan.span(0, n_out)
        base = max(lo, 0)
        raw, scale, x32 = _samples(rng, hi - base, nant, fmt)
        y = la.resample(raw, rate_in, rate_out, n_out=n_out, first_sample=first, first_frac=frac, in_base=base, passband_hz=B, sample_format=fmt, sample_scale=scale,
                        center_offset_hz=off)
        ref, bound = model_resample(off, plan, x32, base, n_out, with_bound=True)
        assert y.shape == (nant, n_out)
        err = np.abs(y.T.astype(np.complex128) - ref)
        lim = ((plan.taps + 2) * 2.0 ** -24 + (2.0 ** -18 if off else 0.0)) * bound
        worst = float(np.max(err / np.maximum(lim, 1e-300)))
        print("wide resample %.2f -> %.2f fmt %d x%d first %d offset %+.0f kHz: T = %d, G = %d, largest error / bound = %.3f" %
              (rate_in / 1e6, rate_out / 1e6, fmt, nant, first, off / 1e3, plan.taps, plan.grp, worst))
        assert plan.grp >= 8 and np.all(err <= lim), worst
        assert float(np.sqrt(np.mean(np.abs(ref) ** 2))) > 0.01    # (the comparison is not one of zeros)


def _gpu(passband, plan, x, in_base, n_out):
    first, frac = plan.start >> 64, (plan.start & (2 ** 64 - 1)) / 2.0 ** 64
    return la.resample(x.astype(np.complex64), plan.rate_in, plan.rate_out, n_out=n_out, first_sample=first, first_frac=frac, in_base=in_base,
                       passband_hz=passband)[0].astype(np.complex128)


@pytest.mark.parametrize("rate_in,rate_out,nof_prb,n_out", [(61.44e6, 5.76e6, 25, 1000), (122.88e6, 3.84e6, 15, 600)])
def test_kernel_meets_the_quality_requirement_on_exact_tones(rate_in, rate_out, nof_prb, n_out, monkeypatch):
    """far into the recording (no output reads the zeros in front of it, so every output counts) and with few outputs: the cost is tones x outputs x ratio.  At
    these ratios several images of one input tone land in band and check_tones resamples the tone once per image: the outputs of a tone are kept"""
    monkeypatch.setattr(resample_cases, "Plan", WidePlan)     # check_tones builds its plan: the wide range's
    seen = {}

    def fn(plan, x, in_base, n):
        key = (x.tobytes(), in_base, n)
        if key not in seen:
            seen[key] = _gpu(passband_hz(nof_prb), plan, x, in_base, n)
        return seen[key]

    worst_pass, worst_land = check_tones(fn, rate_in, rate_out, nof_prb, first_sample=FAR, first_frac=0.25, n_out=n_out)
    print("wide resample GPU %.2f -> %.2f MS/s, %d PRB: pass band %.1f dB, landing in band %.1f dB" %
          (rate_in / 1e6, rate_out / 1e6, nof_prb, 20 * np.log10(worst_pass), 20 * np.log10(max(worst_land, 1e-30))))
    assert worst_pass <= 1e-3 and worst_land <= 1e-3, (worst_pass, worst_land)


@pytest.mark.parametrize("rate_in,rate_out,nof_prb", PAIRS)
def test_one_call_and_the_same_span_in_pieces_are_bit_identical(rate_in, rate_out, nof_prb):
    """pieces of 1, 777 and the rest: a piece starts anywhere in a run and in a round, so an output meets other neighbours in its wavefront - and is the same bits"""
    rng = np.random.default_rng(7)
    B, n_out, first, frac = passband_hz(nof_prb), 3000, 5000, 0.4375
    plan = WidePlan(rate_in, rate_out, B, first, frac)
    lo, hi = plan.span(0, n_out)
    x = (rng.standard_normal((hi - lo, 2)) + 1j * rng.standard_normal((hi - lo, 2))).astype(np.complex64)
    kw = dict(first_sample=first, first_frac=frac, passband_hz=B, center_offset_hz=1e6)
    whole = la.resample(x, rate_in, rate_out, n_out=n_out, in_base=lo, **kw)
    parts = []
    for a, b in ((0, 1), (1, 778), (778, n_out)):
        plo, phi = plan.span(a, b - a)    # each piece is handed only the input it reads
        parts.append(la.resample(x[plo - lo:phi - lo], rate_in, rate_out, n_out=b - a, in_base=plo, out_first=a, **kw))
    assert float(np.abs(whole).max()) > 0 and _same(whole, np.concatenate(parts, axis=1))


RATE = 61.44e6
NARROW = dict(rate_out=30.72e6, passband_hz=passband_hz(100), center_offset_hz=-9.9e6, n_out=1300, first_sample=300, first_frac=0.4375)     # ratio 2
WIDE8 = dict(rate_out=7.68e6, passband_hz=passband_hz(25), center_offset_hz=17e6, n_out=700, first_sample=12345, first_frac=0.5)             # ratio 8: one run and a part
WIDE16 = dict(rate_out=3.84e6, passband_hz=passband_hz(15), center_offset_hz=0.0, n_out=300, first_sample=5000, first_frac=0.0)              # ratio 16: one run and a part


def _single(x, base, c, fmt, scale):
    lo = base
    return la.resample(x, RATE, c["rate_out"], n_out=c["n_out"], first_sample=c["first_sample"], first_frac=c["first_frac"], in_base=lo, passband_hz=c["passband_hz"],
                       sample_format=fmt, sample_scale=scale, center_offset_hz=c["center_offset_hz"])


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_cells_of_both_geometries_in_one_call_equal_the_single_calls(fmt):
    """a ratio-2 cell (512 outputs per run, one lane each) with a ratio-8 and a ratio-16 cell in one lsn_resample_cells call: each equals its own lsn_resample call
    bit for bit, in every order of the cells; and the ratio-2 call gives the same bits before and after the wide-ratio kernels ran"""
    rng = np.random.default_rng(20 + fmt)
    x, scale, _ = _samples(rng, 30000, 2, fmt)
    before = _single(x, 0, NARROW, fmt, scale)
    for cells in ([NARROW, WIDE8], [WIDE8, NARROW], [WIDE16, NARROW, WIDE8], [WIDE8, WIDE16]):
        got = la.resample_cells(x, RATE, cells, in_base=0, sample_format=fmt, sample_scale=scale)
        for c, y in zip(cells, got):
            w = _single(x, 0, c, fmt, scale)
            assert y.shape == (2, c["n_out"]) and float(np.abs(w).max()) > 0 and np.all(np.isfinite(w.view(np.float32))) and _same(y, w), c
    assert _same(_single(x, 0, NARROW, fmt, scale), before)


RING = 32768


@pytest.mark.parametrize("far", [0, FAR - FAR % RING], ids=["near", "2e10_in"])
@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_ring_kernel_equals_the_linear_call_with_the_wrap_anywhere_in_a_run(fmt, far):
    """one ratio-8 cell with 512 outputs - one run, which stages floor(512 * 8) + T + 2 samples - next to a ratio-2 cell.  The end of the ring is put on the first
    staged sample of that run, on its last, inside the T samples in front that it shares with the run before, and at places between; near sample 0 and 2 10^10 in"""
    x, scale, _ = _samples(np.random.default_rng(11 + fmt), 20000, 2, fmt)
    T = la.resample_span(0, 10 ** 9, RATE, 7.68e6, passband_hz=passband_hz(25))["taps"]
    span = 512 * 8 + T + 2
    assert span == WidePlan(RATE, 7.68e6, passband_hz(25)).run_span
    for j in (0, 1, T // 2 - 1, T // 2, T - 1, T, span // 2, span - T, span - 2, span - 1):
        first = far + 5 * RING + T // 2 - 1 - j              # the run stages samples first - T/2 + 1 ...: staged sample j sits at slot 0
        base = first - T // 2 + 1 - 50
        assert (base + 50 + j) % RING == 0
        cells = [dict(WIDE8, n_out=512, first_sample=first, first_frac=0.0), dict(NARROW, first_sample=base + 100)]
        want = la.resample_cells(x, RATE, cells, in_base=base, sample_format=fmt, sample_scale=scale)
        got = la.resample_cells_ring(x, RATE, cells, RING, in_base=base, sample_format=fmt, sample_scale=scale)
        for w, g in zip(want, got):
            assert float(np.abs(w).max()) > 0 and _same(g, w), j


# ---- the recording: a 100-PRB cell at -9.9 MHz and a 25-PRB cell at +17 MHz (ratio 8) in 61.44 MS/s, 12 subframes each ----
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


def _file_pass(raw, jobs, fmt, scale):
    """the bytes written to a file and replayed by process_file_cells -> (subframes done per cell, records per cell)"""
    phys = [_phy(sc, **opt) for sc, opt, _ in jobs]
    try:
        with tempfile.TemporaryDirectory() as td, _block(5):
            path = os.path.join(td, "w.raw")
            raw.tofile(path)
            done = la.process_file_cells(path, WIDE_RATE, [(p, kw) for p, (_, _, kw) in zip(phys, jobs)], sample_format=fmt, sample_scale=scale)
        return done, [gpu_records(p) for p in phys]
    finally:
        for p in phys:
            p.close()


def _stream_pass(raw, jobs, fmt, scale, sizes, **kw):
    phys = [_phy(sc, **opt) for sc, opt, _ in jobs]
    try:
        with _block(16):
            st = la.Stream(WIDE_RATE, [(p, k) for p, (_, _, k) in zip(phys, jobs)], sample_format=fmt, sample_scale=scale, **kw)
        with st:
            pos = 0
            for n in itertools.cycle(sizes):
                if pos >= len(raw):
                    break
                st.push(raw[pos:pos + n])
                pos += n
            done = st.flush()
            status = st.status()
            track = st.track_status() if kw.get("track") is not None else None
            assert status["failed"] == 0 and status["status"] == [0] * len(jobs) and status["samples_pushed"] == len(raw)
        return done, [gpu_records(p) for p in phys], status, track
    finally:
        for p in phys:
            p.close()


@functools.lru_cache(maxsize=None)
def _rec(fmt, strong_db=0.0):
    """computed once per format, shared and left unchanged -> (jobs [(sc, options, the cell's replay arguments)], oracle records per cell, the bytes, scale)"""
    cells, f = wide_recording(strong_db)
    jobs = [(sc, opt, dict(center_offset_hz=f0, start_tti=tti0, offset_time=LEAD, max_subframes=WIDE_NSF)) for sc, tti0, _, opt, f0, _ in cells]
    raw, scale, _ = quantise(f, fmt)
    assert all(len(c[2]) >= 10 for c in cells)
    return jobs, [c[2] for c in cells], raw, scale


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_both_cells_in_one_pass_over_the_file(fmt):
    jobs, orecs, raw, scale = _rec(fmt)
    for order in (1, -1):
        done, got = _file_pass(raw, jobs[::order], fmt, scale)
        assert done == [WIDE_NSF, WIDE_NSF], done
        assert got == orecs[::order], [(len(g), len(o)) for g, o in zip(got, orecs[::order])]


def test_the_narrow_cell_alone_through_process_file_rate():
    jobs, orecs, raw, scale = _rec(la.FILE_CF32)
    sc, opt, kw = jobs[1]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "w.cf32")
        raw.tofile(path)
        for env in ("16", "800"):     # a block buffer of 16 output subframes holds ONE subframe of input at ratio 8; the default holds the whole replay
            with _block(env):
                phy = _phy(sc, **opt)
                try:
                    assert phy.process_file_rate(path, WIDE_RATE, **kw) == WIDE_NSF
                    assert gpu_records(phy) == orecs[1]
                finally:
                    phy.close()


IRREGULAR = (1, 7919, 100003, 33)     # single-sample pushes included


@pytest.mark.parametrize("how", ["one_push", "irregular_blk1", "irregular_blk5", "smallest_ring"])
@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_stream_equals_the_oracle_however_it_is_pushed(fmt, how):
    jobs, orecs, raw, scale = _rec(fmt)
    sizes, kw = {"one_push": ((len(raw),), dict(block_subframes=16)), "irregular_blk1": (IRREGULAR, dict(block_subframes=1)), "irregular_blk5": (IRREGULAR, dict(block_subframes=5)),
                 "smallest_ring": ((61440,), dict(block_subframes=1))}[how]
    if how == "smallest_ring":     # the smallest ring the open accepts for one subframe per block: it wraps several times within the 12 subframes
        need = la.stream_span(WIDE_RATE, [dict(nof_prb=sc["nof_prb"], **k) for sc, _, k in jobs], 0, nof_antennas=2, block_subframes=1)["block_input"]
        kw["ring_samples"] = 1 << (need - 1).bit_length()
        with pytest.raises(ValueError):
            _stream_pass(raw[:10], jobs, fmt, scale, (10,), block_subframes=1, ring_samples=kw["ring_samples"] // 2)
    done, got, status, _ = _stream_pass(raw, jobs, fmt, scale, sizes, **kw)
    assert done == [WIDE_NSF, WIDE_NSF], done
    assert got == orecs, [(len(g), len(o)) for g, o in zip(got, orecs)]
    if how == "smallest_ring":
        assert status["ring_samples"] == kw["ring_samples"] and status["samples_pushed"] > 2 * status["ring_samples"]


def test_tracked_stream_at_zero_clock_error_changes_no_record():
    """the timing loop on and a clock that is right: the tracked segments pass their own step and span, the lanes per output stay the plan's - the oracle's records"""
    jobs, orecs, raw, scale = _rec(la.FILE_CF32)
    done, got, _, ts = _stream_pass(raw, jobs, la.FILE_CF32, scale, IRREGULAR, block_subframes=5, track=dict())
    print("track status, wide recording: %r" % (ts,))
    assert done == [WIDE_NSF, WIDE_NSF] and got == orecs, (done, [len(g) for g in got])
    assert all(ts["segments"][c] >= 3 and ts["valid"][c] >= 2 and ts["lost"][c] == 0 for c in range(2))


def test_the_neighbour_20_db_stronger_with_the_channel_filter():
    """recording (c): the file pass and the stream with stopband_hz from cells_stopbands on both cells"""
    jobs, orecs, raw, scale = _rec(la.FILE_CF32, 20.0)
    stops = la.cells_stopbands([kw["center_offset_hz"] for _, _, kw in jobs], [sc["nof_prb"] for sc, _, _ in jobs], WIDE_RATE)
    filtered = [(sc, opt, dict(kw, stopband_hz=s)) for (sc, opt, kw), s in zip(jobs, stops)]
    done, got = _file_pass(raw, filtered, la.FILE_CF32, scale)
    assert done == [WIDE_NSF, WIDE_NSF] and got[1] == orecs[1], (done, len(got[1]), len(orecs[1]))
    done, again, _, _ = _stream_pass(raw, filtered, la.FILE_CF32, scale, IRREGULAR, block_subframes=3)
    assert done == [WIDE_NSF, WIDE_NSF] and again == got


def test_chain_from_the_carrier_scan_into_one_pass():
    """file_carrier_scan -> carrier_mib -> process_file_cells: neither an offset nor a bandwidth is given by the test; the narrow cell it finds replays"""
    jobs, orecs, raw, scale = _rec(la.FILE_CF32)
    by_offset = {kw["center_offset_hz"]: (sc, opt, kw, o) for (sc, opt, kw), o in zip(jobs, orecs)}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "w.cf32")
        raw.tofile(path)
        found = la.file_carrier_scan(path, WIDE_RATE, nof_antennas=raw.shape[1], nof_periods=1)
        assert sorted(c.center_offset_hz for c in found) == sorted(by_offset)
        chain, want = [], []
        for c in found:
            sc, opt, kw, o = by_offset[c.center_offset_hz]
            mib = la.carrier_mib(la.carrier_channel(raw, WIDE_RATE, c.center_offset_hz), c.search)
            assert mib is not None and c.search.cell_id == sc["cell_id"] and mib["nof_prb"] == sc["nof_prb"]
            chain.append((dict(sc, nof_prb=mib["nof_prb"], nof_ports=mib["nof_ports"], cell_id=int(c.search.cell_id), cp=int(c.search.cp)), opt, dict(kw, center_offset_hz=c)))
            want.append(o)
        phys = [_phy(sc, **opt) for sc, opt, _ in chain]
        try:
            with _block(16):
                done = la.process_file_cells(path, WIDE_RATE, [(p, kw) for p, (_, _, kw) in zip(phys, chain)])
            got = [gpu_records(p) for p in phys]
        finally:
            for p in phys:
                p.close()
    assert done == [WIDE_NSF, WIDE_NSF] and got == want, (done, [len(g) for g in got])


def test_refusals_decode_nothing_and_leave_the_phy_usable():
    jobs, orecs, raw, scale = _rec(la.FILE_CF32)
    sc, opt, kw = jobs[1]
    L = la.lib()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "w.cf32")
        raw.tofile(path)
        phy = _phy(sc, **opt)
        try:
            fc = la.FileCfg(sc["nof_rx"], LEAD, 0.0, la.FILE_CF32, 0.0)
            done = C.c_uint64(99)
            size = C.sizeof(la.FileRate)
            for rate in (122.88e6 + 1.0, 130e6, 32.0001 * 7.68e6):     # above 122.88 MS/s; above ratio 32
                assert L.lsn_phy_process_file_rate(phy._h, os.fsencode(path), C.byref(fc), C.byref(la.FileRate(size, 0, rate, 0.0)), kw["start_tti"], 0, 0, C.byref(done)) == INVALID
                assert done.value == 0 and gpu_records(phy) == []
            out = np.zeros(100, dtype=np.complex64)
            x = np.zeros(200000, dtype=np.complex64)
            for rin, rout, B in ((122.88e6, 122.88e6 / 65, 0.3e6), (122.88e6, 1.92e6, passband_hz(6)), (123e6, 7.68e6, passband_hz(25))):     # ratio 65; a 1.92 MS/s output; above 122.88 MS/s
                cfg = la._resample_cfg(1, rin, rout, 0, 0.0, 0, 0, B, la.FILE_CF32, 0.0)
                assert L.lsn_resample(0, x.ctypes.data, 0, len(x), C.byref(cfg), out.ctypes.data, 0, 100) == INVALID
            good = la._resample_cfg(1, 122.88e6, 3.84e6, 0, 0.0, 0, 0, passband_hz(15), la.FILE_CF32, 0.0)
            assert L.lsn_resample(0, x.ctypes.data, 0, len(x), C.byref(good), out.ctypes.data, 0, 100) == 0
            assert phy.process_file_rate(path, WIDE_RATE, **kw) == WIDE_NSF and gpu_records(phy) == orecs[1]
        finally:
            phy.close()

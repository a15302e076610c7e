"""A live wideband stream pushed in host buffers (k_resample_ring; lsn_resample_cells_ring, lsn_stream_*): the kernel against k_resample_cells, bit for
bit, wherever the ring wraps; and the stream against the file pass on the same bytes and against the oracle's records - one push, pieces of every size down to
single samples, a ring that wraps several times, cells of different bandwidth, one cell, a gap, a flush in the middle - and the refusals that need a device.
Nothing here is a tolerance: every comparison is bit identity or record equality."""
import contextlib
import ctypes as C
import functools
import itertools
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from cells_cases import MIXED_NSF, MIXED_RATE, mixed_recording
from ddc_cases import quantise, recording
from parity import gpu_records
from resample_cases import FAR, LEAD
from resample_model import passband_hz

pytestmark = pytest.mark.gpu
PHICH = {1: 0, 3: 1, 6: 2, 12: 3}
INVALID = -2   # LSN_ERROR_INVALID_INPUTS
RATE = 30.72e6
RING = 32768
# the cell sets of test_gpu_cells.py: three rate pairs with a partial run, a full run and three runs; eight cells, the most one launch takes
THREE = (dict(rate_out=7.68e6, passband_hz=passband_hz(25), center_offset_hz=0.0, n_out=511, first_sample=12345, first_frac=0.0),
         dict(rate_out=23.04e6, passband_hz=passband_hz(75), center_offset_hz=4.5e6, n_out=512, first_sample=5000, first_frac=0.5),
         dict(rate_out=30.72e6, passband_hz=passband_hz(100), center_offset_hz=-3.3e6, n_out=1300, first_sample=0, first_frac=0.4375))
EIGHT = tuple(dict(rate_out=r, passband_hz=passband_hz(p), center_offset_hz=f0, n_out=100, first_sample=2000 * i, first_frac=i / 8.0)
              for i, (r, p, f0) in enumerate(((7.68e6, 25, 7.5e6), (15.36e6, 50, -5e6), (23.04e6, 75, 0.0), (30.72e6, 100, 1e6), (7.68e6, 25, -12e6), (15.36e6, 50, 0.0),
                                              (23.04e6, 75, -8e6), (30.72e6, 100, 6e6))))
WRAP = 3 * RING - 7000     # a window that starts here wraps 7000 samples in
FAR_WRAP = FAR - FAR % RING + RING - 7000


def _noise(n, nant, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == la.FILE_CF32:
        return (rng.standard_normal((n, nant)) + 1j * rng.standard_normal((n, nant))).astype(np.complex64), 0.0
    full, dt, scale = ((32767, np.int16, 1.0 / 9000.0), (127, np.int8, 1.0 / 30.0))[fmt - 1]     # not powers of two: the conversion rounds
    return rng.integers(-full, full + 1, (n, nant, 2)).astype(dt), scale


def _shift(cells, first):
    return [dict(c, first_sample=c["first_sample"] + first) for c in cells]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("base", [0, WRAP, WRAP + FAR, FAR_WRAP], ids=["no_wrap", "wrap_7000_in", "second_shifted_by_FAR", "far_and_wraps"])
@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_ring_kernel_is_k_resample_cells_bit_for_bit(fmt, base):
    """the window [base, base + 20 000) of the recording in a ring of 32 768: at its slots from slot 0 on, wrapping 7000 samples in, and ten minutes into the
    recording (sample indices past 2^34, with and without a wrap).  base = 0: the third cell of THREE reads zeros in front of the recording"""
    n_in, nant = 20000, 2
    assert FAR_WRAP > 2 ** 34 and FAR_WRAP % RING == WRAP % RING == RING - 7000
    x, scale = _noise(n_in, nant, fmt, 3 + fmt)
    first = base + 100 if base else 0
    for cells in (_shift(THREE, first), _shift(EIGHT, first)):
        want = la.resample_cells(x, RATE, cells, in_base=base, sample_format=fmt, sample_scale=scale)
        got = la.resample_cells_ring(x, RATE, cells, RING, in_base=base, sample_format=fmt, sample_scale=scale)
        assert len(got) == len(want) == len(cells)
        for c, y, w in zip(cells, got, want):
            assert y.shape == (nant, c["n_out"]) and float(np.abs(w).max()) > 0 and np.all(np.isfinite(w.view(np.float32)))
            assert _same(y, w), c


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_the_wrap_at_every_place_of_a_single_run(fmt):
    """one cell at D = 4/3 with 512 outputs - one run of one workgroup per antenna, which stages floor(512 D) + T + 2 samples.  The end of the ring is put on the
    first staged sample of that run, on its last, and on six positions between"""
    x, scale = _noise(20000, 2, fmt, 11 + fmt)
    T = la.resample_span(0, 10 ** 9, RATE, 23.04e6, passband_hz=passband_hz(75))["taps"]
    span = 512 * 4 // 3 + T + 2
    places = [0, 1, T // 2 - 1, T // 2, span // 2, span - T, span - 2, span - 1]
    assert len(set(places)) == 8
    for j in places:
        first = 5 * RING + T // 2 - 1 - j              # the run stages samples first - T/2 + 1 ...: staged sample j sits at slot 0
        cell = dict(rate_out=23.04e6, passband_hz=passband_hz(75), center_offset_hz=4.5e6, n_out=512, first_sample=first, first_frac=0.0)
        base = first - T // 2 + 1 - 50
        assert (base + 50 + j) % RING == 0
        want = la.resample_cells(x, RATE, [cell], in_base=base, sample_format=fmt, sample_scale=scale)[0]
        got = la.resample_cells_ring(x, RATE, [cell], RING, in_base=base, sample_format=fmt, sample_scale=scale)[0]
        assert float(np.abs(want).max()) > 0 and _same(got, want), j


def test_ring_call_refuses_a_window_longer_than_the_ring_with_the_outputs_untouched():
    L = la.lib()
    x, _ = _noise(20000, 2, la.FILE_CF32, 1)

    def call(ring, n_in=20000):
        cells = list(THREE)
        n = len(cells)
        cfgs = (la.ResampleCfg * n)(*[la._resample_cfg(2, RATE, c["rate_out"], c["first_sample"], c["first_frac"], 0, 0, c["passband_hz"], la.FILE_CF32, 0.0, c["center_offset_hz"])
                                      for c in cells])
        outs = [np.full((2, c["n_out"]), 7 + 7j, dtype=np.complex64) for c in cells]
        rc = L.lsn_resample_cells_ring(0, x.ctypes.data, n_in, ring, cfgs, n, (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_uint64 * n)(*[c["n_out"] for c in cells]))
        return rc, all(np.all(o == 7 + 7j) for o in outs)

    assert call(RING) == (0, False)
    assert call(16384) == (INVALID, True)        # n_in > ring_samples
    assert call(30000) == (INVALID, True) and call(0) == (INVALID, True)     # not a power of two
    assert call(20000) == (INVALID, True)
    assert call(RING) == (0, False)
    with pytest.raises(ValueError):
        la.resample_cells_ring(x, RATE, list(THREE), 16384)


def _phy(sc, batch=8, **kw):
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=batch, pcapwriter=la.PcapWriter(None), **kw)
    assert phy.set_sampling(la.RATES_3GPP)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], PHICH[sc["phich_ng_x6"]], cp=sc.get("cp", 0))
    return phy


@contextlib.contextmanager
def _block(n):
    """LSN_FILE_BLOCK = n inside (every Phy of a stream holds the file source's block buffers: small blocks, as test_gpu_cells.py)"""
    old = os.environ.get("LSN_FILE_BLOCK")
    os.environ["LSN_FILE_BLOCK"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("LSN_FILE_BLOCK", None)
        else:
            os.environ["LSN_FILE_BLOCK"] = old


def _file_pass(raw, rate_in, cells, fmt, scale):
    """the reference: the bytes written to a file and replayed by process_file_cells -> (subframes done per cell, records per cell)"""
    phys = [_phy(sc, **opt) for sc, opt, _ in cells]
    try:
        with tempfile.TemporaryDirectory() as td, _block(16):
            path = os.path.join(td, "s.raw")
            raw.tofile(path)
            done = la.process_file_cells(path, rate_in, [(p, kw) for p, (_, _, kw) in zip(phys, cells)], sample_format=fmt, sample_scale=scale)
        return done, [gpu_records(p) for p in phys]
    finally:
        for p in phys:
            p.close()


def _pieces(raw, sizes):
    """raw cut into consecutive pieces whose lengths cycle through sizes"""
    pos = 0
    for n in itertools.cycle(sizes):
        if pos >= len(raw):
            return
        yield raw[pos:pos + n]
        pos += n


def _stream_pass(raw, rate_in, cells, fmt, scale, sizes, ops=(), **kw):
    """a Stream over the cells, raw pushed in pieces; ops: {piece index: callable(stream)} run in front of that piece -> (flush's counts, records per cell, the
    status in front of the close)"""
    phys = [_phy(sc, **opt) for sc, opt, _ in cells]
    try:
        with _block(16):
            st = la.Stream(rate_in, [(p, k) for p, (_, _, k) in zip(phys, cells)], sample_format=fmt, sample_scale=scale, **kw)
        with st:
            for i, piece in enumerate(_pieces(raw, sizes)):
                if i in ops:
                    piece = ops[i](st, piece)
                if piece is not None:
                    st.push(piece)
            done = st.flush()
            status = st.status()
            assert status["failed"] == 0 and status["status"] == [0] * len(cells) and status["samples_pushed"] == len(raw)
        return done, [gpu_records(p) for p in phys], status
    finally:
        for p in phys:
            p.close()


@functools.lru_cache(maxsize=None)
def _two_cells(fmt):
    """computed once per format, shared and left unchanged -> (cells, oracle records per cell, rate, the bytes, scale, the file pass's records)"""
    a, b = recording("two_cells_a"), recording("two_cells_b")
    assert np.array_equal(a[-1], b[-1]) and a[5] == b[5] == 61.44e6 and min(len(a[2]), len(b[2])) >= 10
    cells = [(r[0], r[4], dict(center_offset_hz=r[7], start_tti=r[1], offset_time=LEAD)) for r in (a, b)]
    raw, scale, _ = quantise(a[-1], fmt)
    done, ref = _file_pass(raw, a[5], cells, fmt, scale)
    assert done == [12, 12]
    return cells, [r[2] for r in (a, b)], a[5], raw, scale, ref


IRREGULAR = (1, 7919, 100003, 33)     # single-sample pushes included


@pytest.mark.parametrize("how", ["one_push", "pieces_61440", "irregular_blk1", "irregular_blk5", "smallest_ring"])
@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_stream_equals_the_file_pass_and_the_oracle(fmt, how):
    """the two 100-PRB cells at +-9.9 MHz of the 61.44 MS/s recording, 12 subframes each, both cell orders: however the bytes are pushed, each Phy's records are
    those of process_file_cells on a file of the same bytes, and the oracle's"""
    cells, orecs, rate_in, raw, scale, ref = _two_cells(fmt)
    assert ref == orecs
    sizes, kw = {"one_push": ((len(raw),), dict(block_subframes=16)), "pieces_61440": ((61440,), dict(block_subframes=4)), "irregular_blk1": (IRREGULAR, dict(block_subframes=1)),
                 "irregular_blk5": (IRREGULAR, dict(block_subframes=5)), "smallest_ring": ((61440,), dict(block_subframes=1))}[how]
    if how == "smallest_ring":     # the smallest ring the open accepts for one subframe per block: the ring wraps several times within the 12 subframes
        need = la.stream_span(rate_in, [dict(nof_prb=100, **k) for _, _, k in cells], 0, nof_antennas=2, block_subframes=1)["block_input"]
        kw["ring_samples"] = 1 << (need - 1).bit_length()
        with pytest.raises(ValueError):
            _stream_pass(raw[:10], rate_in, cells, fmt, scale, (10,), block_subframes=1, ring_samples=kw["ring_samples"] // 2)
    for order in (1, -1):
        done, got, status = _stream_pass(raw, rate_in, cells[::order], fmt, scale, sizes, **kw)
        assert done == [12, 12], done
        assert got == ref[::order] and got == orecs[::order], [len(g) for g in got]
        if how == "smallest_ring":
            assert status["ring_samples"] == kw["ring_samples"] and status["samples_pushed"] > 2 * status["ring_samples"]


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_cells_of_different_bandwidth_in_one_stream(fmt):
    """cells_cases.mixed_recording in irregular pieces: a 75-PRB and a 25-PRB cell of one 30.72 MS/s stream, the 25-PRB cell cut by max_subframes - the counts and
    records test_cells_of_different_bandwidth_in_one_pass asserts of the file pass"""
    cells, f = mixed_recording()
    jobs = [(sc, opt, dict(center_offset_hz=f0, start_tti=tti0, offset_time=LEAD, max_subframes=MIXED_NSF if sc["nof_prb"] == 25 else 0)) for sc, tti0, _, opt, f0, _ in cells]
    raw, scale, _ = quantise(f, fmt)
    done, got, _ = _stream_pass(raw, MIXED_RATE, jobs, fmt, scale, IRREGULAR, block_subframes=3)
    assert done == [MIXED_NSF, MIXED_NSF], done
    for (sc, _, orecs, _, _, _), g in zip(cells, got):
        assert len(orecs) >= 10 and g == orecs, "%d PRB: %d records vs %d" % (sc["nof_prb"], len(g), len(orecs))


def test_one_cell_is_process_file_rate():
    cells, orecs, rate_in, raw, scale, _ = _two_cells(la.FILE_CF32)
    sc, opt, kw = cells[1]
    phy = _phy(sc, **opt)
    try:
        with tempfile.TemporaryDirectory() as td, _block(16):
            path = os.path.join(td, "s.cf32")
            raw.tofile(path)
            n = phy.process_file_rate(path, rate_in, **kw)
        single = gpu_records(phy)
    finally:
        phy.close()
    done, got, _ = _stream_pass(raw, rate_in, [cells[1]], la.FILE_CF32, scale, IRREGULAR, block_subframes=5)
    assert done == [n] == [12] and got == [single] and single == orecs[1]


def test_a_gap_is_the_file_with_those_samples_zeroed():
    """the samples of one subframe in the middle are not pushed: gap(n) stands for them.  Positions stay, zeros arrive: the records are those of the file pass on
    the same bytes with that stretch zeroed"""
    cells, _, rate_in, raw, scale, ref = _two_cells(la.FILE_CF32)
    lo, n = LEAD + 6 * 61440, 61440
    zeroed = raw.copy()
    zeroed[lo:lo + n] = 0
    done_f, want = _file_pass(zeroed, rate_in, cells, la.FILE_CF32, scale)
    assert done_f == [12, 12] and min(len(w) for w in want) >= 10 and want != ref     # the zeroed file still yields that many, and not what the whole one yields

    def gap(st, piece):
        assert len(piece) == n
        st.gap(n)
        return None
    done, got, status = _stream_pass(raw, rate_in, cells, la.FILE_CF32, scale, (lo, n, 200000), ops={1: gap}, block_subframes=2)
    assert done == [12, 12] and got == want and min(len(g) for g in got) >= 10


def test_a_flush_in_the_middle_changes_nothing():
    cells, orecs, rate_in, raw, scale, ref = _two_cells(la.FILE_SC16)
    seen = []

    def flush(st, piece):
        seen.extend([st.flush(), st.flush(), st.status()["samples_pushed"]])
        return piece
    done, got, _ = _stream_pass(raw, rate_in, cells, la.FILE_SC16, scale, IRREGULAR, ops={10: flush}, block_subframes=5)
    mid, again, pushed = seen
    inside = (pushed - LEAD) % 61440
    assert 1000 < inside < 60000                                   # the piece in front of the flush ended inside a subframe ...
    assert mid == again == [(pushed - LEAD) // 61440] * 2 and 0 < mid[0] < 12 and mid[0] % 5     # ... and the flush submitted every complete one, no whole number of blocks
    assert done == [12, 12] and got == ref and got == orecs


def test_refusals_allocate_nothing_and_leave_every_phy_usable():
    cells, orecs, rate_in, raw, scale, _ = _two_cells(la.FILE_CF32)
    (sa, oa, ka), (sb, ob, kb) = cells
    with tempfile.TemporaryDirectory() as td, _block(16):
        path = os.path.join(td, "s.cf32")
        raw.tofile(path)
        pa, pb = _phy(sa, **oa), _phy(sb, **ob)
        multi = la.Phy(nof_rx_antennas=2, max_batch=4, pcapwriter=la.PcapWriter(None), devices=[0, 0])
        assert multi.setCell(sb["nof_prb"], sb["nof_ports"], sb["cell_id"], PHICH[sb["phich_ng_x6"]])
        one = la.Phy(nof_rx_antennas=1, max_batch=4, pcapwriter=la.PcapWriter(None))
        assert one.setCell(100, 2, 9)
        try:
            assert pb.set_channel_filter(10.5e6)
            with pytest.raises(ValueError):                           # a Phy with a channel filter set: refused, not dropped
                la.Stream(rate_in, [(pa, ka), (pb, kb)])
            assert pb.set_channel_filter(0.0)
            for bad in ([(pa, ka), (multi, kb)],                       # a lsn_phy_create_multi handle
                        [(pa, ka), (one, kb)],                         # a Phy with another antenna count than the stream's
                        [(pa, ka), (pa, kb)],                          # a Phy twice
                        [(pa, ka), (pb, dict(kb, start_tti=la.TTI_FROM_MIB))]):
                with pytest.raises(ValueError):
                    la.Stream(rate_in, bad, nof_antennas=2)
            with pytest.raises(ValueError):
                la.Stream(rate_in, [(pa, ka), (pb, kb)], nof_antennas=1)     # antenna-count mismatch
            with la.Stream(rate_in, [(pa, ka)], block_subframes=4) as held:
                with pytest.raises(ValueError):                       # a Phy already in an open stream
                    la.Stream(rate_in, [(pb, kb), (pa, ka)])
                assert held.flush() == [0]
            st = la.Stream(rate_in, [(pa, ka), (pb, kb)], block_subframes=4)     # the close gave the Phy back
            assert st.close() == [0, 0] and st.close() is None
            with pytest.raises(ValueError):                           # push, gap and flush after close
                st.push(raw[:100])
            with pytest.raises(ValueError):
                st.gap(5)
            with pytest.raises(ValueError):
                st.flush()
            assert gpu_records(pa) == [] and gpu_records(pb) == []
            for phy, kw, o in ((pa, ka, orecs[0]), (pb, kb, orecs[1])):
                assert phy.process_file_rate(path, rate_in, **kw) == 12
                assert gpu_records(phy) == o
        finally:
            for p in (pa, pb, multi, one):
                p.close()

"""A live stream with the channel filter on (k_chan_fir_ring; lsn_channel_filter_ring, lsn_stream_* on Phys with lsn_phy_set_channel_filter): the ring
kernel against k_chan_fir bit for bit wherever the ring wraps; the filtered stream against the filtered file pass on the same bytes and against the oracle's records
on the recordings whose neighbour carrier is 20 dB stronger - one push, pieces down to single samples, the smallest ring, both formats, one cell, a gap, a flush in
the middle -; the same with the timing loop on, against the expectation tests/test_stream_filter_plan.py establishes with the float64 chain; and the refusals that
need a device.  Nothing here is a tolerance: every comparison is bit identity or record equality."""
import ctypes as C
import functools
import itertools
import os
import tempfile

import numpy as np
import pytest

import ltesniffer_amd as la
from chanfilt_cases import B100, NSF, RATE, STOP, quantise, recording
from parity import gpu_records
from resample_cases import LEAD
from resample_model import passband_hz
from stream_filter_cases import DRIFT_STOP
from test_gpu_stream import IRREGULAR, _block, _file_pass, _noise, _phy, _pieces, _same, _stream_pass
from test_gpu_track import _phys, _track_pass
from track_cases import DRIFT_LEAD, DRIFT_NSF, drifting_recording, record_tti

pytestmark = pytest.mark.gpu
INVALID = -2   # LSN_ERROR_INVALID_INPUTS
RING = 8192
TILE = 1024
# (pass band, stop band) -> L = 8, 88, 512
G8, G88, G512 = (B100, RATE / 2), (B100, STOP), (B100, B100 + 0.0049 * RATE)
FAR = 20_000_000_000 - 20_000_000_000 % RING      # a window that starts at slot 0, 2 x 10^10 samples into the recording (indices past 2^34)
WRAP = 3 * RING - 2000                              # a window that starts here wraps 2000 samples in


def _cell(g, f0, first, n_out):
    return dict(passband_hz=g[0], stopband_hz=g[1], center_offset_hz=f0, out_first=first, n_out=n_out)


# one cell (a launch out of a ring is the ring kernel's also for one), three, and eight - the most one launch takes - with different n_out, one of them 0; outputs
# of 1023, 1024, 1025 and 3079 samples off the tile grid.  out_first is counted from the window's first sample + 512, so every cell's span lies in a window of 6000
ONE = (_cell(G88, 9.9e6, 333, 3079),)
THREE = (_cell(G8, 0.0, 777, TILE - 1), _cell(G512, -9.9e6, 100, TILE + 1), _cell(G88, 9.9e6, 1501, TILE))
EIGHT = (_cell(G88, 9.9e6, 0, 3079), _cell(G8, 0.0, 1, TILE), _cell(G512, 9.9e6, 2, 0), _cell(G512, 0.0, 3, 3079), _cell(G88, -9.9e6, 1025, TILE + 1),
         _cell(G8, -9.9e6, 4000, TILE - 1), _cell(G88, 0.0, 17, 1), _cell(G512, -9.9e6, 2047, 2 * TILE + 5))


def _at(cells, first):
    return [dict(c, out_first=c["out_first"] + first) for c in cells]


@pytest.mark.parametrize("base", [0, WRAP, FAR, FAR + WRAP], ids=["slot_0", "wraps_2000_in", "far_slot_0", "far_and_wraps"])
@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_ring_kernel_is_k_chan_fir_bit_for_bit(fmt, base):
    """the window [base, base + 6000) of the recording in a ring of 8192 whose other slots hold NaN patterns.  base = 0: the cells' first outputs read the zeros in
    front of the recording"""
    assert FAR % RING == 0 and FAR > 2 ** 34 and (FAR + WRAP) % RING == WRAP % RING == RING - 2000
    for nant in (1, 2):
        x, scale = _noise(6000, nant, fmt, 5 + fmt + nant)
        for cells in (ONE, THREE, EIGHT):
            cells = _at(cells, base + 512 if base else 0)
            got = la.channel_filter_ring(x, RATE, cells, RING, in_base=base, sample_format=fmt, sample_scale=scale)
            assert len(got) == len(cells)
            for c, y in zip(cells, got):
                assert y.shape == (c["n_out"], nant)
                if not c["n_out"]:
                    continue
                want = la.channel_filter(x, RATE, c["passband_hz"], c["stopband_hz"], n_out=c["n_out"], center_offset_hz=c["center_offset_hz"], in_base=base,
                                         out_first=c["out_first"], sample_format=fmt, sample_scale=scale)
                assert float(np.abs(want).max()) > 0 and np.all(np.isfinite(want.view(np.float32)))
                assert _same(y, want), c


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16, la.FILE_SC8])
def test_the_wrap_at_every_place_of_a_tile(fmt):
    """one cell, L = 88, 1024 outputs: one tile of one workgroup per antenna, which stages 1024 + 2 L = 1200 samples.  The end of the ring is put on the first staged
    sample, on the last, and on six places between - quad boundaries (multiples of four) and the middle of a quad among them"""
    x, scale = _noise(6000, 2, fmt, 21 + fmt)
    L, need = 88, TILE + 2 * 88
    places = [0, 2, 4, 255, 256, 601, need - 4, need - 1]
    assert len(set(places)) == 8 and {p % 4 for p in places} == {0, 1, 2, 3}
    for j in places:
        first = 5 * RING + L - j                  # the tile stages samples first - L ...: staged sample j sits at slot 0
        base = first - L - 50
        assert (base + 50 + j) % RING == 0
        c = _cell(G88, 9.9e6, first, TILE)
        want = la.channel_filter(x, RATE, *G88, n_out=TILE, center_offset_hz=9.9e6, in_base=base, out_first=first, sample_format=fmt, sample_scale=scale)
        got = la.channel_filter_ring(x, RATE, [c], RING, in_base=base, sample_format=fmt, sample_scale=scale)[0]
        assert float(np.abs(want).max()) > 0 and _same(got, want), j


def test_the_door_refuses_a_window_longer_than_the_ring_with_the_outputs_untouched():
    L = la.lib()
    x, _ = _noise(6000, 2, la.FILE_CF32, 1)

    def call(ring, n_in=6000, cells=THREE):
        cells = _at(cells, 512)
        n = len(cells)
        cfgs = (la.ChannelFilterCfg * n)(*[la._channel_filter_cfg(2, RATE, c["passband_hz"], c["stopband_hz"], c["center_offset_hz"], 0, c["out_first"], la.FILE_CF32, 0.0)
                                           for c in cells])
        outs = [np.full((c["n_out"], 2), 7 + 7j, dtype=np.complex64) for c in cells]
        rc = L.lsn_channel_filter_ring(0, x.ctypes.data, n_in, ring, cfgs, n, (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_uint64 * n)(*[c["n_out"] for c in cells]))
        return rc, all(np.all(o == 7 + 7j) for o in outs)

    assert call(RING) == (0, False)
    assert call(4096) == (INVALID, True)                                      # n_in > ring_samples
    assert call(6000) == (INVALID, True) and call(0) == (INVALID, True)       # not a power of two
    assert call(1 << 33) == (INVALID, True)                                   # the ring mask is 32 bits wide
    # whatever lsn_channel_filter refuses: S <= B, L > 512, and outputs whose input the window does not hold
    assert call(RING, cells=(THREE[0], _cell((B100, B100), 0.0, 0, 10))) == (INVALID, True)
    assert call(RING, cells=(THREE[0], _cell((B100, B100 + 100e3), 0.0, 0, 10))) == (INVALID, True)
    assert call(RING, cells=(THREE[0], _cell(G88, 0.0, 5000, 1000))) == (INVALID, True)
    assert call(RING) == (0, False)
    with pytest.raises(ValueError) as err:
        la.channel_filter_ring(x, RATE, _at(THREE, 512), 4096)
    assert all(not o.any() for o in err.value.outs)


# ---- records: the recording whose other carrier is 20 dB stronger, both cells, stopband_hz from cells_stopbands ----

@functools.lru_cache(maxsize=None)
def _strong(fmt):
    """computed once per format, shared and left unchanged -> (cells with the filter, the same cells without it, oracle records per cell, the bytes, scale, the
    filtered file pass's records).  The first cell (B) is the weak one"""
    b, a = recording("b_wanted"), recording("a_wanted")
    stops = la.cells_stopbands([-9.9e6, 9.9e6], [100, 100], RATE)
    assert stops == [STOP, STOP] and b[5] == RATE
    plain = [(r[0], r[4], dict(center_offset_hz=f0, start_tti=r[1], offset_time=LEAD)) for r, f0 in ((b, -9.9e6), (a, 9.9e6))]
    cells = [(sc, opt, dict(k, stopband_hz=s)) for (sc, opt, k), s in zip(plain, stops)]
    raw, scale, _ = quantise(b[-1], fmt)
    done, ref = _file_pass(raw, RATE, cells, fmt, scale)
    assert done == [NSF, NSF]
    return cells, plain, [b[2], a[2]], raw, scale, ref


def _off(cells):
    """the cells with the filter switched off on their Phys (the setting is sticky: a dict without stopband_hz would leave what an earlier open set)"""
    return [(sc, opt, dict(k, stopband_hz=0.0)) for sc, opt, k in cells]


@pytest.mark.parametrize("how", ["one_push", "pieces_61440", "irregular_blk1", "irregular_blk5", "smallest_ring"])
@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_filtered_stream_equals_the_filtered_file_pass_and_the_oracle(fmt, how):
    cells, plain, orecs, raw, scale, ref = _strong(fmt)
    assert ref == orecs and sorted(len(o) for o in orecs) == [66, 69]
    sizes, kw = {"one_push": ((len(raw),), dict(block_subframes=16)), "pieces_61440": ((61440,), dict(block_subframes=4)), "irregular_blk1": (IRREGULAR, dict(block_subframes=1)),
                 "irregular_blk5": (IRREGULAR, dict(block_subframes=5)), "smallest_ring": ((61440,), dict(block_subframes=1))}[how]
    if how == "smallest_ring":     # the smallest ring the open accepts for one subframe per block: it wraps several times within the 12 subframes
        need = la.stream_span(RATE, [dict(nof_prb=100, **{k: v for k, v in c[2].items() if k != "stopband_hz"}) for c in cells], 0, nof_antennas=2, block_subframes=1,
                              stopbands=[STOP, STOP])["block_input"]
        kw["ring_samples"] = 1 << (need - 1).bit_length()
        with pytest.raises(ValueError):
            _stream_pass(raw[:10], RATE, cells, fmt, scale, (10,), block_subframes=1, ring_samples=kw["ring_samples"] // 2)
    for order in (1, -1):
        done, got, status = _stream_pass(raw, RATE, cells[::order], fmt, scale, sizes, **kw)
        assert done == [NSF, NSF], done
        assert got == ref[::order] and got == orecs[::order], [len(g) for g in got]
        if how == "smallest_ring":
            assert status["ring_samples"] == kw["ring_samples"] and status["samples_pushed"] > 2 * status["ring_samples"]


def test_the_filter_is_what_passes_and_switching_it_off_gives_todays_records():
    """the same stream with the filter off decodes fewer records of the weak cell than the oracle has - and exactly what the unfiltered file pass decodes: today's
    records.  Then on Phys that had the filter on before: a filtered stream is decoded on them (the setting switched to 0.0 while it is open: it stays as it was
    opened), and with the setting at 0.0 a stream is RE-OPENED on the same Phys - intermediates reserved, back on the one-launch k_resample_ring path - and decodes
    what the unfiltered path decodes on such Phys.  The yardstick of that second decode is the file pass with the same history on Phys of its own (a filtered
    process_file_cells, then an unfiltered one): a Phy keeps its RNTI and MCS state from one decode to the next, so it is not the records of fresh Phys.  Those are
    what Phys give that were only SET UP for two stages (a filtered stream opened and closed without a sample) and then re-opened with the setting at 0.0"""
    cells, plain, orecs, raw, scale, _ = _strong(la.FILE_CF32)
    done_f, today = _file_pass(raw, RATE, _off(cells), la.FILE_CF32, scale)
    done, got, _ = _stream_pass(raw, RATE, _off(cells), la.FILE_CF32, scale, IRREGULAR, block_subframes=5)
    print("filter off: %r records, the oracle has %r" % ([len(g) for g in got], [len(o) for o in orecs]))
    assert done == done_f == [NSF, NSF] and got == today
    assert len(got[0]) < len(orecs[0]) and got[0] != orecs[0]
    with _phys(cells) as fphys, tempfile.TemporaryDirectory() as td, _block(16):      # the file pass with the same history: filter on, then off
        path = os.path.join(td, "s.cf32")
        raw.tofile(path)
        assert la.process_file_cells(path, RATE, [(p, k) for p, (_, _, k) in zip(fphys, cells)]) == [NSF, NSF]
        assert [gpu_records(p) for p in fphys] == orecs
        for p in fphys:
            p.pcapwriter.reset()
        assert la.process_file_cells(path, RATE, [(p, k) for p, (_, _, k) in zip(fphys, _off(cells))]) == [NSF, NSF]
        again = [gpu_records(p) for p in fphys]
    print("filter off behind a filtered decode on the same Phys: %r records (fresh Phys: %r)" % ([len(g) for g in again], [len(g) for g in today]))
    with _phys(cells) as phys:
        with _block(16):
            for p, (_, _, k) in zip(phys, cells):
                assert p.set_channel_filter(k["stopband_hz"])
            with la.Stream(RATE, [(p, k) for p, (_, _, k) in zip(phys, plain)], block_subframes=4) as st:      # (opens filtered: the setting is the Phy's)
                # the setting of a Phy of an open stream counts for the next open: this stream stays as it was opened
                assert all(p.set_channel_filter(0.0) for p in phys)
                st.push(raw)
                assert st.flush() == [NSF, NSF]
            assert [gpu_records(p) for p in phys] == orecs
            for p in phys:
                p.pcapwriter.reset()
            # re-open on the same Phys, the setting now 0.0
            with la.Stream(RATE, [(p, k) for p, (_, _, k) in zip(phys, plain)], block_subframes=5) as st:
                for piece in _pieces(raw, IRREGULAR):
                    st.push(piece)
                assert st.flush() == [NSF, NSF]
            reopened = [gpu_records(p) for p in phys]
            # (not `today`: behind a decode the Phys know the cell's RNTIs from the first subframe on - measured: 65 and 75 records against 64 and 69 - and the file
            # pass with the same history says the same, record for record)
            assert reopened == again, ([len(g) for g in reopened], [len(g) for g in again])
            assert reopened[0] != orecs[0] and len(reopened[0]) < len(orecs[0])      # the weak cell still loses records without the filter
            for p in phys:
                p.pcapwriter.reset()
    # and on Phys that were set up for two stages but have decoded nothing: a filtered stream is opened on them (taps uploaded, intermediate reserved) and closed
    # without a sample, the setting goes to 0.0, the stream is re-opened: exactly the records of fresh Phys
    with _phys(cells) as phys, _block(16):
        with la.Stream(RATE, [(p, k) for p, (_, _, k) in zip(phys, cells)], block_subframes=4) as st:
            assert st.flush() == [0, 0]
        assert all(p.set_channel_filter(0.0) for p in phys)
        with la.Stream(RATE, [(p, k) for p, (_, _, k) in zip(phys, plain)], block_subframes=5) as st:
            for piece in _pieces(raw, IRREGULAR):
                st.push(piece)
            assert st.flush() == [NSF, NSF]
        fresh = [gpu_records(p) for p in phys]
        assert fresh == today and len(fresh[0]) < len(orecs[0]), ([len(g) for g in fresh], [len(g) for g in today])


def test_a_flushed_stream_has_submitted_what_file_cells_span_counts_for_a_file_of_n_samples():
    """the plan with Phys (file_cells_span reads the filter's setting from a Phy, so this check needs them; no kernel runs): filter off and on, over every fourth
    value of the CPU plan test's grid and the places where L decides, with two block sizes"""
    cells, plain, _, raw, _, _ = _strong(la.FILE_CF32)
    with _phys(cells) as phys:
        grid = sorted(set(list(range(0, len(raw), 4 * 4099)) + [0, 1, 87, 88, 89, LEAD + 61440 + 60, LEAD + 61440 + 60 + 88, LEAD + 61440 + 60 + 89, len(raw) - 1, len(raw)]))
        for stop in (0.0, STOP):
            assert all(p.set_channel_filter(stop) for p in phys)
            pc = [(p, k) for p, (_, _, k) in zip(phys, plain)]
            for blk_sf in (5, 16):
                for N in grid:
                    tot = [0, 0]
                    for blk in range(100):
                        b = la.file_cells_span(RATE, pc, N, block=blk, blk_subframes=blk_sf, nof_antennas=2)
                        if not b["nof_active"]:
                            break
                        tot = [t + n for t, n in zip(tot, b["nof_subframes"])]
                    assert la.stream_span(RATE, pc, N, nof_antennas=2, block_subframes=blk_sf)["subframes_complete"] == tot, (stop, blk_sf, N)


def test_nobody_grows_the_intermediate_under_an_open_filtered_stream():
    """the stream's launches write and read the Phy's filter intermediate.  lsn_phy_prepare_file with a larger LSN_FILE_BLOCK would free and reallocate it: refused
    while the stream is open, and the stream decodes the oracle's records; after the close the same call goes through"""
    cells, _, orecs, raw, scale, _ = _strong(la.FILE_CF32)
    with _phys(cells) as phys:
        with _block(16):
            st = la.Stream(RATE, [(p, k) for p, (_, _, k) in zip(phys, cells)], block_subframes=4)
        with st:
            st.push(raw[:200000])
            with _block(64):
                for p in phys:
                    with pytest.raises(RuntimeError):
                        p.prepare_file()
            st.push(raw[200000:])
            assert st.flush() == [NSF, NSF]
        assert [gpu_records(p) for p in phys] == orecs
        with _block(64):
            for p in phys:
                p.prepare_file()


def test_one_filtered_cell_is_process_file_rate_with_the_filter():
    cells, _, orecs, raw, scale, _ = _strong(la.FILE_CF32)
    sc, opt, kw = cells[0]
    phy = _phy(sc, **opt)
    try:
        with tempfile.TemporaryDirectory() as td, _block(16):
            path = os.path.join(td, "s.cf32")
            raw.tofile(path)
            assert phy.set_channel_filter(kw["stopband_hz"])
            n = phy.process_file_rate(path, RATE, **{k: v for k, v in kw.items() if k != "stopband_hz"})
        single = gpu_records(phy)
    finally:
        phy.close()
    done, got, _ = _stream_pass(raw, RATE, [cells[0]], la.FILE_CF32, scale, IRREGULAR, block_subframes=5)
    assert done == [n] == [NSF] and got == [single] and single == orecs[0]


def test_a_gap_is_the_filtered_file_with_those_samples_zeroed():
    cells, _, _, raw, scale, ref = _strong(la.FILE_CF32)
    lo, n = LEAD + 6 * 61440, 61440
    zeroed = raw.copy()
    zeroed[lo:lo + n] = 0
    done_f, want = _file_pass(zeroed, RATE, cells, la.FILE_CF32, scale)
    assert done_f == [NSF, NSF] and min(len(w) for w in want) >= 10 and want != ref

    def gap(st, piece):
        assert len(piece) == n
        st.gap(n)
        return None
    done, got, _ = _stream_pass(raw, RATE, cells, la.FILE_CF32, scale, (lo, n, 200000), ops={1: gap}, block_subframes=2)
    assert done == [NSF, NSF] and got == want


def test_a_flush_inside_a_subframe_changes_nothing():
    cells, _, orecs, raw, scale, ref = _strong(la.FILE_SC16)
    seen = []

    def flush(st, piece):
        seen.extend([st.flush(), st.flush(), st.status()["samples_pushed"]])
        return piece
    done, got, _ = _stream_pass(raw, RATE, cells, la.FILE_SC16, scale, IRREGULAR, ops={10: flush}, block_subframes=5)
    mid, again, pushed = seen
    assert 1000 < (pushed - LEAD) % 61440 < 60000                                # the piece in front of the flush ended inside a subframe ...
    assert mid == again == [(pushed - LEAD) // 61440] * 2 and 0 < mid[0] < NSF and mid[0] % 5     # ... and the flush submitted every complete one
    assert done == [NSF, NSF] and got == ref and got == orecs


# ---- tracked ----

@pytest.mark.parametrize("how", ["one_push_blk16", "irregular_blk5", "irregular_blk1"])
def test_tracked_and_filtered_next_to_the_strong_neighbour(how):
    """case (a) of tests/test_stream_filter_plan.py: the clock is right, the loop on.  The float64 chain decodes every record of the oracle, so the GPU has to"""
    cells, _, orecs, raw, scale, _ = _strong(la.FILE_CF32)
    sizes, kw = {"one_push_blk16": ((len(raw),), dict(block_subframes=16)), "irregular_blk5": (IRREGULAR, dict(block_subframes=5)),
                 "irregular_blk1": (IRREGULAR, dict(block_subframes=1))}[how]
    done, got, _, ts = _track_pass(raw, RATE, cells, la.FILE_CF32, scale, sizes, dict(), **kw)
    print("tracked + filtered (%s): %r" % (how, ts))
    assert done == [NSF, NSF] and got == orecs, [len(g) for g in got]
    assert all(v >= 2 for v in ts["valid"]) and ts["lost"] == [0, 0] and all(abs(e) < 8.0 for e in ts["last_error"])


def _drift_filtered(sizes, ring_samples=0, block_subframes=16, track=None):
    """the drifting recording through a one-cell filtered, tracked Stream (initial_ppm = 60) -> (count, records, the loop's status behind the flush)"""
    sc, tti0, _, opt, rate, f = drifting_recording()
    with _phys([(sc, opt, None)]) as phys:
        with _block(16):
            st = la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD, stopband_hz=DRIFT_STOP))], block_subframes=block_subframes, ring_samples=ring_samples,
                           track=dict(initial_ppm=60.0) if track is None else track)
        with st:
            pos = 0
            for n in itertools.cycle(sizes):
                if pos >= len(f):
                    break
                st.push(f[pos:pos + n])
                pos += n
            done = st.flush()
            ts = st.track_status()
            assert st.status()["failed"] == 0 and st.status()["samples_pushed"] == len(f)
        return done[0], gpu_records(phys[0]), ts


def test_tracked_and_filtered_on_a_drifting_clock():
    """case (b): S = 3.5 MHz (L = 21), initial_ppm = 60.  Pushed whole, and in 1 ms pieces through the smallest ring lsn_stream_track accepts: every record of the
    oracle, and records, the loop's whole status and position_drift (a double, with ==) equal between the two"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    assert la.channel_filter_design(rate, passband_hz(25), DRIFT_STOP)["L"] == 21 and len(orecs) == 1040
    ring = 1024
    with _phys([(sc, opt, None)]) as phys:
        while True:
            try:
                with _block(16):
                    st = la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD, stopband_hz=DRIFT_STOP))], block_subframes=1, ring_samples=ring)
            except ValueError:
                ring *= 2
                continue
            with st:
                try:
                    st.track(initial_ppm=60.0)
                    break
                except ValueError:
                    ring *= 2
    assert ring == 16384            # one subframe of 10 000 samples, the resampler's span and 2 x 21
    n0, want, ts0 = _drift_filtered((1 << 40,))
    n, got, ts = _drift_filtered((10000,), ring_samples=ring, block_subframes=1)
    print("drifting + filtered: %d subframes, %d of %d records; status %r" % (n0, len(want), len(orecs), ts0))
    assert n0 >= DRIFT_NSF and [r for r in want if record_tti(r) < tti0 + DRIFT_NSF] == orecs
    assert n == n0 and got == want
    assert ts == ts0 and ts["position_drift"][0] == ts0["position_drift"][0] != 0.0, (ts, ts0)
    assert ts["lost"] == [0] and ts["invalid"] == [0] and 75.0 < ts["correction_ppm"][0] < 85.0


# ---- refusals that need a device, each followed by a successful decode on the same Phys ----

def _late(cells, samples):
    return [cells[0], (cells[1][0], cells[1][1], dict(cells[1][2], offset_time=cells[1][2]["offset_time"] + samples))]


@pytest.mark.parametrize("what", ["mix", "L_above_512", "S_not_above_B", "tti_from_mib", "ring_below_the_widened_block", "track_ring_with_2L"])
def test_a_refusal_allocates_nothing_and_the_same_phys_decode_afterwards(what):
    cells, plain, orecs, raw, scale, _ = _strong(la.FILE_CF32)
    kw = [k for _, _, k in cells]
    flat = [dict(nof_prb=100, **{a: v for a, v in k.items() if a != "stopband_hz"}) for k in kw]
    need = la.stream_span(RATE, flat, 0, nof_antennas=2, block_subframes=1, stopbands=[STOP, STOP])["block_input"]
    with _phys(cells) as phys, _block(16):
        def refused(ks, **open_kw):
            with pytest.raises(ValueError):
                la.Stream(RATE, list(zip(phys, ks)), **open_kw)
        if what == "mix":
            refused([kw[0], dict(kw[1], stopband_hz=0.0)])
            refused([dict(kw[0], stopband_hz=0.0), dict(kw[1], stopband_hz=STOP)])
        elif what == "L_above_512":
            refused([kw[0], dict(kw[1], stopband_hz=B100 + 100e3)])
        elif what == "S_not_above_B":
            refused([kw[0], dict(kw[1], stopband_hz=B100)])
            refused([kw[0], dict(kw[1], stopband_hz=RATE / 2 + 1.0)])
        elif what == "tti_from_mib":
            refused([kw[0], dict(kw[1], start_tti=la.TTI_FROM_MIB)])
        elif what == "ring_below_the_widened_block":
            # the second cell starts so much later that one block of both ends 3 samples short of 65 536 WITHOUT the filter: the unfiltered stream opens on that
            # ring, the filtered one - 2 x 88 samples more - does not
            assert need - 176 < 65536 - 16
            late = _late(cells, 65536 - (need - 176) - 3)
            refused([k for _, _, k in late], block_subframes=1, ring_samples=65536)
            la.Stream(RATE, [(p, dict(k, stopband_hz=0.0)) for p, (_, _, k) in zip(phys, late)], block_subframes=1, ring_samples=65536).close()
        else:
            # one block of both cells WITH the filter ends 3 samples short of the ring: the stream opens; at 120 ppm a subframe widens by 7 samples and track is
            # refused - without the 2 L in its check it would be accepted, the plain block being 176 samples shorter -, at 10 ppm (0.6 samples) it is accepted
            late = _late(cells, 65536 - need - 3)
            for tight, ok in ((dict(max_ppm=120.0), False), (dict(max_ppm=10.0), True)):
                with la.Stream(RATE, [(p, k) for p, (_, _, k) in zip(phys, late)], block_subframes=1, ring_samples=65536) as st:
                    if ok:
                        st.track(**tight)
                    else:
                        with pytest.raises(ValueError):
                            st.track(**tight)
                    assert st.flush() == [0, 0]
        assert [gpu_records(p) for p in phys] == [[], []]
        with la.Stream(RATE, list(zip(phys, kw)), block_subframes=4) as st:
            st.push(raw)
            assert st.flush() == [NSF, NSF]
        assert [gpu_records(p) for p in phys] == orecs

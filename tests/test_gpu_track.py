"""The timing loop of a pushed stream on the GPU (k_pss_timing; lsn_pss_timing, lsn_stream_track): the detector kernel against the float64 model within
the float32 dot-product bound and bit for bit against itself, a tracked stream at zero clock error against the oracle's records, and the refusals that need a
device."""
import contextlib
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import ltesniffer_amd as la
import track_model as tm
from parity import gpu_records
from test_gpu_stream import IRREGULAR, _phy, _block, _two_cells
from track_cases import DRIFT_LEAD, DRIFT_NSF, blocks, drifting_recording, record_tti, rep

pytestmark = pytest.mark.gpu
INVALID = -2   # LSN_ERROR_INVALID_INPUTS


def _cell(N, offsets, nant, cfo_hz=0.0, snr_db=30.0):
    d, p = tm.lag_spacing(N), tm.pss_index(N)
    return dict(blocks=blocks(N, offsets, nant, snr_db, cfo_hz), occ=[(i, p) for i in range(len(offsets))], replica=rep(N, cfo_hz), d=d)


def _check(cell, got):
    """every value within the bound of the float32 evaluation; -> the largest error / bound"""
    worst = 0.0
    x, r, d = cell["blocks"], cell["replica"], cell["d"]
    for (sf, p), g in zip(cell["occ"], got):
        want, bound = tm.corr13(x[sf], p, r, d, with_bound=True)
        assert np.all(np.isfinite(g))
        if not np.any(x[sf]):
            assert np.all(g == 0.0)          # a subframe of zeros: every denominator is 0, no NaN
            continue
        err = np.abs(g.astype(np.float64) - want)
        assert np.all(err <= bound), (sf, p, err / bound)
        worst = max(worst, float(np.max(err / bound)))
    return worst


@pytest.mark.parametrize("nant", [1, 2])
@pytest.mark.parametrize("N", [128, 512, 2048])
def test_kernel_against_the_model_within_the_dot_product_bound(N, nant):
    """a PSS at p, at p +- 6 d (the window's edges), at a fractional offset, and a subframe of zeros.  |C_gpu - C_model| <= the bound track_model.corr13 derives:
    (N + 3) 2^-24 times the sum of magnitudes of each dot product, through the square and the quotient.  Largest error / bound seen on an MI355X: DESIGN 3.1h"""
    d = tm.lag_spacing(N)
    offsets = [0.0, 6.0 * d, -6.0 * d, 1.37 * d, None]
    cell = _cell(N, offsets, nant, cfo_hz=2000.0 if nant == 2 else 0.0)
    got = la.pss_timing([cell])[0]
    assert got.shape == (5, 13) and got.dtype == np.float32
    ratio = _check(cell, got)
    print("k_pss_timing N %d, %d antenna(s): largest error / bound = %.4f" % (N, nant, ratio))
    # where the peak lies: lag 6, lag 12, lag 0, between lags 7 and 8
    assert [int(np.argmax(g)) for g in got[:4]] == [6, 12, 0, 7]
    ok, e, _ = la.pss_timing_error(got[3], d)
    assert ok and abs(e - 1.37 * d) < 0.5 * d
    assert la.pss_timing_error(got[1], d)[0] is False and la.pss_timing_error(got[4], d)[0] is False


def test_two_cells_of_different_size_in_one_launch_and_bit_identity():
    """a 6-PRB cell with two antennas and a 100-PRB cell with one in ONE launch: each within its bound; the same call twice, and the same occurrences one launch
    each, give the same bits"""
    a = _cell(128, [0.0, -2.5, 3.2, None], 2)
    b = _cell(2048, [16.0 * 1.75, 0.0], 1, cfo_hz=2000.0)
    got = la.pss_timing([a, b])
    assert got[0].shape == (4, 13) and got[1].shape == (2, 13)
    _check(a, got[0])
    _check(b, got[1])
    again = la.pss_timing([a, b])
    for g, h in zip(got, again):
        assert np.array_equal(g.view(np.uint32), h.view(np.uint32))
    for cell, g in ((a, got[0]), (b, got[1])):
        for i, occ in enumerate(cell["occ"]):
            single = la.pss_timing([dict(cell, occ=[occ])])[0]
            assert np.array_equal(single.view(np.uint32), g[i:i + 1].view(np.uint32)), (cell["d"], i)
    # more than four occurrences of a cell go out four per launch: the same bits again
    many = dict(a, occ=a["occ"] * 3)
    assert np.array_equal(la.pss_timing([many])[0].view(np.uint32), np.tile(got[0], (3, 1)).view(np.uint32))


def _track_pass(raw, rate_in, cells, fmt, scale, sizes, track, **kw):
    """_stream_pass of test_gpu_stream.py with the timing loop on -> (counts, records per cell, the stream's status, the loop's status behind the flush)"""
    phys = [_phy(sc, **opt) for sc, opt, _ in cells]
    try:
        with _block(16):
            st = la.Stream(rate_in, [(p, k) for p, (_, _, k) in zip(phys, cells)], sample_format=fmt, sample_scale=scale, track=track, **kw)
        with st:
            pos = 0
            for n in itertools.cycle(sizes):
                if pos >= len(raw):
                    break
                st.push(raw[pos:pos + n])
                pos += n
            done = st.flush()
            status = st.status()
            seen = st.track_status()
            assert status["failed"] == 0 and status["status"] == [0] * len(cells) and status["samples_pushed"] == len(raw)
        return done, [gpu_records(p) for p in phys], status, seen
    finally:
        for p in phys:
            p.close()


@pytest.mark.parametrize("how", ["one_push_blk16", "irregular_blk5", "pieces_blk1"])
def test_tracking_at_zero_clock_error_changes_no_record(how):
    """the two-cell 12-subframe recording of test_gpu_stream.py with the loop on and a clock that is right: both Phys' records are the oracle's, the counts
    [12, 12], and the loop has seen its PSS - however the stream is pushed"""
    cells, orecs, rate_in, raw, scale, ref = _two_cells(la.FILE_CF32)
    sizes, kw = {"one_push_blk16": ((len(raw),), dict(block_subframes=16)), "irregular_blk5": (IRREGULAR, dict(block_subframes=5)),
                 "pieces_blk1": ((61440,), dict(block_subframes=1))}[how]
    done, got, status, ts = _track_pass(raw, rate_in, cells, la.FILE_CF32, scale, sizes, dict(), **kw)
    assert done == [12, 12], done
    assert got == orecs and got == ref, [len(g) for g in got]
    print("track status at zero clock error (%s): %r" % (how, ts))
    for c, (_, _, k) in enumerate(cells):
        nseg = ts["segments"][c]
        assert 3 <= nseg <= 4 and ts["valid"][c] + ts["invalid"][c] >= nseg - 1 and ts["valid"][c] >= 2 and ts["lost"][c] == 0
        # N = 2048: d = 16.  Below d / 2 the right lag was picked; a correction is at most (Kp + 4 Ki) e per segment of 153 600 samples, and three of them moved
        # the position (in input samples, two per output sample)
        assert abs(ts["last_error"][c]) < 8.0 and abs(ts["correction_ppm"][c]) < 0.375 * 8.0 / 153600 * 1e6 and abs(ts["position_drift"][c]) < 3 * 0.375 * 8.0 * 2


def test_status_does_not_depend_on_the_pushes():
    """the loop's whole state behind the flush, position_drift compared as a double with ==, across one push, irregular pieces and every block size"""
    cells, orecs, rate_in, raw, scale, _ = _two_cells(la.FILE_CF32)
    runs = [_track_pass(raw, rate_in, cells, la.FILE_CF32, scale, sizes, dict(initial_ppm=3.0), block_subframes=b)
            for sizes, b in (((len(raw),), 16), (IRREGULAR, 5), ((61440,), 1), ((30720,), 16))]
    for done, got, _, ts in runs[1:]:
        assert done == runs[0][0] and got == runs[0][1] and ts == runs[0][3], (ts, runs[0][3])
    assert runs[0][3]["position_drift"][0] != 0.0      # 3 ppm of 12 subframes at 61.44 MS/s: a few samples off the nominal plan


@contextlib.contextmanager
def _phys(cells):
    phys = [_phy(sc, **opt) for sc, opt, _ in cells]
    try:
        yield phys
    finally:
        for p in phys:
            p.close()


def test_refusals_leave_the_stream_usable():
    cells, orecs, rate_in, raw, scale, _ = _two_cells(la.FILE_CF32)
    need = la.stream_span(rate_in, [dict(nof_prb=100, **k) for _, _, k in cells], 0, nof_antennas=2, block_subframes=1)["block_input"]
    with _phys(cells) as phys:
        with _block(16):
            st = la.Stream(rate_in, [(p, k) for p, (_, _, k) in zip(phys, cells)], block_subframes=1, ring_samples=1 << (need - 1).bit_length())
        with st:
            cfg = la._track_cfg(2)
            cfg.struct_size -= 4
            assert la.lib().lsn_stream_track(st._h, C.byref(cfg)) == INVALID            # a size-off struct_size
            for bad in (dict(kp=-1.0), dict(ki=float("nan")), dict(max_ppm=121.0), dict(max_ppm=50.0, initial_ppm=60.0), dict(initial_ppm=[0.0, -101.0]),
                        dict(cfo_hz=float("inf"))):
                with pytest.raises(ValueError):
                    st.track(**bad)
            with pytest.raises(ValueError):
                st.track_status()                                               # not tracking
            st.push(raw[:1000])
            with pytest.raises(ValueError):
                st.track()                                                       # after a push
            st.push(raw[1000:])
            assert st.flush() == [12, 12]
        assert [gpu_records(p) for p in phys] == orecs                          # the stream decoded, untracked
    # a ring that holds the nominal block and not the widened one (one subframe at 61.44 MS/s widens by 7 samples at 120 ppm, by 0.6 at 10 ppm): the second
    # cell is started so much later that one block of both cells ends 3 samples short of 65536.  The stream opens, track is refused at 120 ppm and accepted at
    # 10 ppm, and cell 0 - the one that starts on its subframe - decodes the oracle's records either way
    assert need < 65536 - 16
    late = [cells[0], (cells[1][0], cells[1][1], dict(cells[1][2], offset_time=cells[1][2]["offset_time"] + 65536 - need - 3))]
    assert la.stream_span(rate_in, [dict(nof_prb=100, **k) for _, _, k in late], 0, nof_antennas=2, block_subframes=1, ring_samples=65536)["block_input"] == 65533
    for tight, ok in ((dict(max_ppm=120.0), False), (dict(max_ppm=10.0), True)):
        with _phys(late) as phys:
            with _block(16):
                st = la.Stream(rate_in, [(p, k) for p, (_, _, k) in zip(phys, late)], block_subframes=1, ring_samples=65536)
            with st:
                if ok:
                    st.track(**tight)
                else:
                    with pytest.raises(ValueError):
                        st.track(**tight)
                st.push(raw)
                assert st.flush()[0] == 12
            assert gpu_records(phys[0]) == orecs[0]


# ---- the reason for the loop: a recording whose clock is off by 60 ppm and slews to 80 ppm (track_cases.drifting_recording) ----
# tests/test_track_model.py checks, without a GPU, what makes these meaningful: replayed open loop the oracle loses nearly every record, resampled with the model
# loop it finds every record from segment 40 on.

def _drift_pass(sizes, track, gap=None, ring_samples=0, block_subframes=16, mid=None):
    """the drifting recording through a one-cell Stream -> (count, records, the loop's status behind the flush [, what mid(stream) returned at each of its calls])"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    seen = []
    with _phys([(sc, opt, None)]) as phys:
        with _block(16):
            st = la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD))], block_subframes=block_subframes, ring_samples=ring_samples, track=track)
        with st:
            pos = 0
            for n in itertools.cycle(sizes):
                if pos >= len(f):
                    break
                n = min(n, len(f) - pos)
                if gap and gap[0] <= pos < gap[1]:
                    n = min(n, gap[1] - pos)
                    st.gap(n)
                else:
                    if gap and pos < gap[0]:
                        n = min(n, gap[0] - pos)
                    st.push(f[pos:pos + n])
                pos += n
                while mid and len(seen) < len(mid) and pos >= mid[len(seen)]:      # the first piece that reaches each of the places in mid
                    st.flush()
                    seen.append(st.track_status())
            done = st.flush()
            ts = st.track_status() if track is not None else None
            assert st.status()["failed"] == 0 and st.status()["samples_pushed"] == len(f)
        return done[0], gpu_records(phys[0]), ts, seen


@functools.lru_cache(maxsize=None)
def _drift_whole():
    """the tracked pass pushed whole: computed once, shared by the tests below"""
    return _drift_pass((1 << 40,), dict())


def test_a_drifting_clock_is_followed():
    """without track the stream loses records; with it, from the first subframe of segment 40 on, it gives exactly the oracle's records, and in front of that none
    that differs; with initial_ppm = 60 every record of the recording is there"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    first = tti0 + 200
    late = [r for r in orecs if record_tti(r) >= first]
    n_open, open_loop, _, _ = _drift_pass((1 << 40,), None)
    print("open loop: %d subframes, %d of %d records" % (n_open, len(open_loop), len(orecs)))
    assert len(open_loop) < len(orecs)
    n, got, ts, _ = _drift_whole()
    early = [r for r in got if record_tti(r) < first]
    print("tracked: %d subframes, %d of %d records (%d in front of segment 40); status %r" % (n, len(got), len(orecs), len(early), ts))
    assert n >= DRIFT_NSF
    assert [r for r in got if first <= record_tti(r) < tti0 + DRIFT_NSF] == late
    assert set(early) <= set(orecs)
    assert ts["lost"] == [0] and ts["invalid"] == [0] and 75.0 < ts["correction_ppm"][0] < 85.0      # the clock ends at 80 ppm
    n, got, ts, _ = _drift_pass((1 << 40,), dict(initial_ppm=60.0))
    assert [r for r in got if record_tti(r) < tti0 + DRIFT_NSF] == orecs


@pytest.mark.parametrize("how", ["pieces_1ms", "irregular", "smallest_ring", "blk1", "blk5"])
def test_records_and_the_loop_do_not_depend_on_how_the_stream_is_pushed(how):
    """against the recording pushed whole with blocks of 16: in 1 ms pieces, in pieces cycling through 1, 7919, 100 003 and 33 samples, through the smallest ring
    lsn_stream_track accepts, with blocks of 1 and 5 subframes - records and the loop's whole status equal, position_drift compared as a double with =="""
    n0, want, ts0, _ = _drift_whole()
    kw = dict(pieces_1ms=dict(sizes=(10000,)), irregular=dict(sizes=IRREGULAR), smallest_ring=dict(sizes=(10000,), block_subframes=1),
              blk1=dict(sizes=(1 << 40,), block_subframes=1), blk5=dict(sizes=(1 << 40,), block_subframes=5))[how]
    if how == "smallest_ring":
        sc, tti0, _, opt, rate, _ = drifting_recording()
        ring = 1024
        with _phys([(sc, opt, None)]) as phys:
            while True:
                try:
                    with _block(16):
                        st = la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD))], block_subframes=1, ring_samples=ring)
                except ValueError:
                    ring *= 2
                    continue
                with st:
                    try:
                        st.track()
                        break
                    except ValueError:
                        ring *= 2
        assert ring == 16384        # one subframe of 10 000 samples and the filter's span
        kw["ring_samples"] = ring
    n, got, ts, _ = _drift_pass(kw.pop("sizes"), dict(), **kw)
    assert n == n0 and got == want
    assert ts == ts0, (ts, ts0)


def test_a_gap_over_three_half_frames_holds_the_rate():
    """gap() over 15 ms in the middle (the PSS subframes 200, 205 and 210 lie inside): three measurements are invalid, the correction does not move across them, and
    every record behind the last subframe the gap touches is the oracle's"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    lo = DRIFT_LEAD + int(199.5 * 10000 * (1.0 + 70e-6))
    hi = lo + 150000
    # the loop's status inside segment 41 (subframes 205 .. 209: entered with the last measurement taken in front of the gap, that of segment 39) and inside segment 44
    # (220 .. 224: entered with the third invalid one, that of segment 42).  Segments 42, 43 and 44 run at c = I, and I has not moved
    at = [DRIFT_LEAD + int(sf * 10000 * (1.0 + 70e-6)) for sf in (207.5, 222.5)]
    n, got, ts, seen = _drift_pass((10000,), dict(), gap=(lo, hi), mid=at)
    assert len(seen) == 2
    print("gap: status in segment 41 %r, in segment 44 %r, at the end %r" % (seen[0], seen[1], ts))
    assert seen[0]["segments"] == [42] and seen[1]["segments"] == [45]
    assert seen[0]["invalid"] == [2] and seen[1]["invalid"] == [3] and ts["invalid"] == [3] and ts["valid"] == [77] and ts["lost"] == [0]
    assert seen[1]["integrator_ppm"] == seen[0]["integrator_ppm"]                      # held exactly
    assert seen[1]["correction_ppm"] == seen[1]["integrator_ppm"]                      # invalid: c = I
    assert 65.0 < seen[1]["correction_ppm"][0] < 75.0                                  # the clock is at 70 ppm there
    clear = tti0 + 216
    assert [r for r in got if clear <= record_tti(r) < tti0 + DRIFT_NSF] == [r for r in orecs if record_tti(r) >= clear]
    assert not [r for r in got if tti0 + 200 <= record_tti(r) < tti0 + 214]             # nothing decodes inside the gap

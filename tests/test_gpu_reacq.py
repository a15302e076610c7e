"""Re-acquisition of a tracked stream on the GPU (k_pss_acquire; lsn_pss_acquire, lsn_stream_reacquire): the search kernel against the float64 model
within the float32 dot-product bound and bit for bit against k_pss_timing and itself, the three cut recordings of reacq_cases through a stream - however it is
pushed - against the oracle's records and the figures of the CPU round trip (tests/test_reacq_model.py), and the refusals that need a device."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import ltesniffer_amd as la
import reacq_model as rq
import track_model as tm
from parity import gpu_records
from reacq_cases import CUT_AFTER, CUT_JUMP_SEGMENT, CUT_OFFSETS, CUT_PPM, CUTS, cut_recording, span
from test_gpu_stream import IRREGULAR, _block, _two_cells
from test_gpu_track import _phys
from track_cases import DRIFT_LEAD, DRIFT_NSF, drifting_recording, record_tti, rep

pytestmark = pytest.mark.gpu
INVALID = -2   # LSN_ERROR_INVALID_INPUTS
CUT_RECORDS, CUT_LATE = 933, 882      # the CPU round trip's: records in all, and from segment 12's TTI on (every one of the oracle's)


# ---- the kernel ----

def _places(N):
    """where the PSS of the kernel test's span lie: at lag 0; at a fractional place in the second subframe; straddling the boundary between subframes 2 and 3; at
    the last lag, whose window crosses into subframe 5, the sixth"""
    d = tm.lag_spacing(N)
    return [0.0, 20.0 * N + 0.37 * d, 45.0 * N - N // 2, 75.0 * N - d]


@functools.lru_cache(maxsize=None)
def _span_cell(N, nant):
    return dict(blocks=span(N, _places(N), nant, cfo_hz=2000.0 if nant == 2 else 0.0), replica=rep(N, 2000.0 if nant == 2 else 0.0), d=tm.lag_spacing(N))


@pytest.mark.parametrize("nant", [1, 2])
@pytest.mark.parametrize("N", [128, 512, 2048])
def test_kernel_against_the_model_within_the_dot_product_bound(N, nant):
    """one span with four PSS - at lag 0, at a fractional place, straddling a subframe boundary, at the last lag (its window reaches into the sixth subframe) -
    and a span of zeros.  |C_gpu - C_model| <= the bound of track_model.corr13 at every one of the 9600 lags: (N + 3) 2^-24 times the sum of magnitudes of each
    dot product, through the square and the quotient.  The 13 values around p in each of the first five subframes equal k_pss_timing's with =="""
    d, p = tm.lag_spacing(N), tm.pss_index(N)
    cell = _span_cell(N, nant)
    zeros = dict(cell, blocks=np.zeros_like(cell["blocks"]))
    got, gz = la.pss_acquire([cell, zeros])
    assert got.shape == (9600,) and got.dtype == np.float32 and np.all(np.isfinite(got))
    assert np.all(gz == 0.0)                                # every denominator is 0: no NaN
    want, bound = rq.metric(cell["blocks"], cell["replica"], d, with_bound=True)
    err = np.abs(got.astype(np.float64) - want)
    print("k_pss_acquire N %d, %d antenna(s): largest error / bound = %.4f" % (N, nant, float(np.max(err / bound))))
    assert np.all(err <= bound), float(np.max(err / bound))
    # the four PSS are the four largest local maxima, each at the lag next to its place
    for at in _places(N):
        i = int(round(at / d))
        lo, hi = max(i - 40, 0), min(i + 41, 9600)
        assert abs(lo + int(np.argmax(got[lo:hi])) - at / d) <= 0.5 and got[i] > 4.0 * np.median(got)
    # bit identity with k_pss_timing: subframe s of the span, window around p <-> lags (s sflen + p) / d - 6 .. + 6
    timing = la.pss_timing([dict(cell, occ=[(s, p) for s in range(5)])])[0]
    for s in range(5):
        i = (s * 15 * N + p) // d
        assert np.array_equal(timing[s].view(np.uint32), got[i - 6:i + 7].view(np.uint32)), (N, nant, s)


def test_two_cells_of_different_size_in_one_launch_and_bit_identity():
    """a 6-PRB cell with two antennas and a 100-PRB cell with one in ONE launch; the same call twice, and each cell in a launch of its own: the same bits"""
    a, b = _span_cell(128, 2), _span_cell(2048, 1)
    got = la.pss_acquire([a, b])
    again = la.pss_acquire([a, b])
    alone = [la.pss_acquire([a])[0], la.pss_acquire([b])[0]]
    swapped = la.pss_acquire([b, a])[::-1]
    for g, h, k, m in zip(got, again, alone, swapped):
        assert np.array_equal(g.view(np.uint32), h.view(np.uint32)) and np.array_equal(g.view(np.uint32), k.view(np.uint32))
        assert np.array_equal(g.view(np.uint32), m.view(np.uint32))
    for cell, g in ((a, got[0]), (b, got[1])):
        ok, o, peak, ratio = la.pss_acquire_decide(g, cell["d"], len(cell["replica"]))
        assert (ok, o, peak, ratio) == rq.decide(g.astype(np.float64), cell["d"], len(cell["replica"]))


# ---- the cut recordings through a stream ----

def _pass(f, sizes, track, reacquire, ring_samples=0, block_subframes=16, gap=None, mid=()):
    """a recording [sample][antenna] through a one-cell Stream -> (count, records, track_status, reacquire_status or None).  gap: (lo, hi), the samples of the
    recording that arrive as a declared gap; mid: places at which - behind the first piece that reaches them - the stream is flushed and both statuses are asked"""
    sc, tti0, orecs, opt, rate, _ = drifting_recording()
    with _phys([(sc, opt, None)]) as phys:
        with _block(16):
            st = la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD))], block_subframes=block_subframes, ring_samples=ring_samples, track=track,
                           reacquire=reacquire)
        with st:
            pos = seen = 0
            for n in itertools.cycle(sizes):
                if pos >= len(f):
                    break
                if gap and gap[0] <= pos < gap[1]:
                    n = min(n, gap[1] - pos)
                    st.gap(n)
                else:
                    n = min(n, len(f) - pos, gap[0] - pos if gap and pos < gap[0] else n)
                    st.push(f[pos:pos + n])
                pos += n
                while seen < len(mid) and pos >= mid[seen]:
                    st.flush()
                    st.track_status()
                    st.reacquire_status()
                    seen += 1
            done = st.flush()
            ts = st.track_status()
            rs = st.reacquire_status() if reacquire is not None else None
            assert st.status()["failed"] == 0 and st.status()["samples_pushed"] == len(f)
        return done[0], gpu_records(phys[0]), ts, rs


TRACK, REACQ = dict(initial_ppm=CUT_PPM), dict(after=CUT_AFTER)


@functools.lru_cache(maxsize=None)
def _cut_whole(name):
    """a cut recording pushed whole with blocks of 16: computed once, shared by the tests below"""
    return _pass(cut_recording(name), (1 << 40,), TRACK, REACQ)


@pytest.mark.parametrize("name", list(CUTS))
def test_a_cut_recording_is_found_again(name):
    """3000 samples removed, 17 001 removed, 9000 duplicated at input sample DRIFT_LEAD + 200 000: one search, accepted, the offset that of the CPU round trip (the
    cut times 96 / 125), the jump in force at segment 12; from that segment's TTI on the records are exactly the oracle's, in front of it none differs, and the
    count is the round trip's"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    n, got, ts, rs = _cut_whole(name)
    print("%s: %d subframes, %d records; track %r; reacquire %r" % (name, n, len(got), ts, rs))
    assert rs["launched"] == [1] and rs["accepted"] == [1] and rs["rejected"] == [0]
    assert rs["last_offset"] == [CUT_OFFSETS[name]] and rs["jump_segment"] == [CUT_JUMP_SEGMENT]
    assert rs["last_ratio"][0] >= rq.MIN_RATIO and abs(rs["jumps_total"][0] - CUTS[name]) < 4 * 125.0 / 96.0 + 1.0      # the jump in input samples: the cut, within d
    first = tti0 + 5 * CUT_JUMP_SEGMENT
    late = [r for r in orecs if record_tti(r) >= first]
    assert len(late) == CUT_LATE
    assert [r for r in got if first <= record_tti(r) < tti0 + DRIFT_NSF] == late
    assert set(r for r in got if record_tti(r) < first) <= set(orecs)
    assert len([r for r in got if record_tti(r) < tti0 + DRIFT_NSF]) == CUT_RECORDS
    assert ts["lost"] == [0] and ts["invalid"] == [8]       # segments 4 .. 11


def _smallest_ring():
    """the smallest ring lsn_stream_reacquire accepts for blocks of one subframe"""
    sc, tti0, _, opt, rate, _ = drifting_recording()
    ring, refused_by_reacquire = 1024, 0
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
                    st.track(**TRACK)
                except ValueError:
                    ring *= 2
                    continue
                try:
                    st.reacquire(**REACQ)
                    return ring, refused_by_reacquire
                except ValueError:
                    refused_by_reacquire += 1
                    ring *= 2


@pytest.mark.parametrize("how", ["pieces_1ms", "irregular", "smallest_ring", "blk1", "blk5"])
@pytest.mark.parametrize("name", list(CUTS))
def test_records_and_both_statuses_do_not_depend_on_how_the_stream_is_pushed(name, how):
    """against the cut recording pushed whole with blocks of 16: in 1 ms pieces, in pieces cycling through 1, 7919, 100 003 and 33 samples, through the smallest
    ring lsn_stream_reacquire accepts, with blocks of 1 and 5 subframes - records, track_status and reacquire_status equal, the doubles compared with =="""
    n0, want, ts0, rs0 = _cut_whole(name)
    kw = dict(pieces_1ms=dict(sizes=(10000,)), irregular=dict(sizes=IRREGULAR), smallest_ring=dict(sizes=(10000,), block_subframes=1),
              # (the default ring of blocks of one subframe, four blocks, does not hold the 8 subframes a searched cell keeps: lsn_stream_reacquire refuses it)
              blk1=dict(sizes=(1 << 40,), block_subframes=1, ring_samples=1 << 18), blk5=dict(sizes=(1 << 40,), block_subframes=5))[how]
    if how == "smallest_ring":
        ring, refused = _smallest_ring()
        # one subframe of 10 000 samples and the filter's span need 16 384 (lsn_stream_track's smallest); 8 subframes more, 80 008 samples at 100 ppm: 131 072
        assert ring == 131072 and refused == 3
        kw["ring_samples"] = ring
    n, got, ts, rs = _pass(cut_recording(name), kw.pop("sizes"), TRACK, REACQ, **kw)
    assert n == n0 and got == want
    assert ts == ts0 and rs == rs0, (ts, ts0, rs, rs0)


@pytest.mark.parametrize("sizes", [(1 << 40,), (10000,)])
def test_a_search_whose_span_reads_a_gap_is_not_launched(sizes):
    """3000 samples removed as above, and 5000 samples in the middle of the span of segment 9 (subframes 45 .. 50) declared as a gap: the search that is due at
    segment 9 is not launched and counts as rejected when segment 12 is entered, the next one is due there and then, is launched and accepted, and the jump is in
    force at segment 15 - by the same offset, within d (the loop holds its rate in between).  Every record from segment 15's TTI on is the oracle's"""
    sc, tti0, orecs, opt, rate, _ = drifting_recording()
    lo = DRIFT_LEAD + 470000
    n, got, ts, rs = _pass(cut_recording("removed_3000"), sizes, TRACK, REACQ, gap=(lo, lo + 5000))
    print("gap in the span of segment 9: track %r; reacquire %r" % (ts, rs))
    assert rs["launched"] == [1] and rs["accepted"] == [1] and rs["rejected"] == [1] and rs["jump_segment"] == [CUT_JUMP_SEGMENT + 3]
    assert abs(rs["last_offset"][0] - CUT_OFFSETS["removed_3000"]) <= 4
    first = tti0 + 5 * (CUT_JUMP_SEGMENT + 3)
    assert [r for r in got if first <= record_tti(r) < tti0 + DRIFT_NSF] == [r for r in orecs if record_tti(r) >= first]
    assert set(r for r in got if record_tti(r) < first) <= set(orecs)


def test_flushes_and_status_calls_in_between_change_nothing():
    """a flush and both status calls every 3 ms from the subframe in which the search becomes due (45) to the segment behind the jump: the status calls take
    measurements and the search's result in early, and records and both statuses at the end are still those of the recording pushed whole"""
    n0, want, ts0, rs0 = _cut_whole("removed_17001")
    mid = tuple(DRIFT_LEAD + 440000 + 30000 * i + 4321 for i in range(8))
    n, got, ts, rs = _pass(cut_recording("removed_17001"), (10000,), TRACK, REACQ, mid=mid)
    assert n == n0 and got == want and ts == ts0 and rs == rs0, (ts, ts0, rs, rs0)


def test_without_a_cut_nothing_is_searched_and_nothing_changes():
    """re-acquisition on and no loss: the records and the loop's status are those of the same stream without it, and no search was launched"""
    f = drifting_recording()[5]
    n0, want, ts0, _ = _pass(f, (1 << 40,), TRACK, None)
    n, got, ts, rs = _pass(f, (1 << 40,), TRACK, REACQ)
    assert n == n0 and got == want and ts == ts0
    assert rs["launched"] == [0] and rs["accepted"] == [0] and rs["rejected"] == [0] and rs["jump_segment"] == [0] and rs["jumps_total"] == [0.0]
    assert [r for r in got if record_tti(r) < drifting_recording()[1] + DRIFT_NSF] == drifting_recording()[2]      # every record of the recording


def test_without_reacquire_the_cut_recording_stays_lost():
    """what the feature is for: the same cut recording through a stream that only tracks decodes nothing behind the cut"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    n, got, ts, _ = _pass(cut_recording("removed_3000"), (1 << 40,), dict(initial_ppm=CUT_PPM, lost_after=CUT_AFTER), None)
    behind = [r for r in got if record_tti(r) >= tti0 + 5 * CUT_JUMP_SEGMENT]
    print("tracked, no re-acquisition: %d records, %d from segment 12 on; %r" % (len(got), len(behind), ts))
    assert ts["lost"] == [1] and ts["valid"] == [4]         # segments 0 .. 3, in front of the cut
    # what a stream gives today: the records in front of the cut - those the re-acquiring stream has in front of its jump (933 - 882 = 51) - and none behind
    assert not behind and len(got) == CUT_RECORDS - CUT_LATE and set(got) <= set(orecs)


# ---- refusals ----

def test_refusals_leave_the_stream_usable():
    cells, orecs, rate_in, raw, scale, _ = _two_cells(la.FILE_CF32)
    open_kw = dict(block_subframes=1)

    def stream(phys, **kw):
        with _block(16):
            return la.Stream(rate_in, [(p, k) for p, (_, _, k) in zip(phys, cells)], **dict(open_kw, **kw))
    with _phys(cells) as phys:
        with stream(phys) as st:
            with pytest.raises(ValueError):
                st.reacquire()                                                   # an untracked stream
            with pytest.raises(ValueError):
                st.reacquire_status()
            st.track()
            cfg = la._reacquire_cfg(2)
            cfg.struct_size += 8
            assert la.lib().lsn_stream_reacquire(st._h, C.byref(cfg)) == INVALID  # a size-off struct_size
            for bad in (dict(min_ratio=0.99), dict(min_ratio=float("nan")), dict(min_ratio=float("inf")), dict(min_ratio=-3.0), dict(enable=[True])):
                with pytest.raises(ValueError):
                    st.reacquire(**bad)
            with pytest.raises(ValueError):
                st.reacquire_status()                                            # not re-acquiring
            st.push(raw[:1000])
            with pytest.raises(ValueError):
                st.reacquire()                                                   # after a push
            st.push(raw[1000:])
            assert st.flush() == [12, 12]
        assert [gpu_records(p) for p in phys] == orecs
    # a ring that holds what lsn_stream_track asks for and not the 8 subframes more (491 520 samples at 61.44 MS/s): track is accepted, reacquire refused
    need = la.stream_span(rate_in, [dict(nof_prb=100, **k) for _, _, k in cells], 0, nof_antennas=2, block_subframes=1)["block_input"]
    ring = 1 << (need + 1024).bit_length()
    assert ring < 491520
    with _phys(cells) as phys:
        with stream(phys, ring_samples=ring) as st:
            st.track()
            with pytest.raises(ValueError):
                st.reacquire()
            st.push(raw)
            assert st.flush() == [12, 12]
        assert [gpu_records(p) for p in phys] == orecs
    # accepted - one call only -, and twelve subframes with nothing lost: no search, the oracle's records
    with _phys(cells) as phys:
        with stream(phys, ring_samples=1 << 20, track=dict(), reacquire=dict(after=1, enable=[True, False])) as st:
            with pytest.raises(ValueError):
                st.reacquire()
            st.push(raw)
            assert st.flush() == [12, 12]
            rs = st.reacquire_status()
            assert rs["launched"] == [0, 0] and rs["rejected"] == [0, 0]
        assert [gpu_records(p) for p in phys] == orecs


def test_a_filtered_stream_is_refused_and_decodes():
    """the two-stage filtered path is left out: lsn_stream_reacquire refuses, and the stream - filtered and tracked - gives every record of the recording"""
    from stream_filter_cases import DRIFT_STOP
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    with _phys([(sc, opt, None)]) as phys:
        with _block(16):
            st = la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD, stopband_hz=DRIFT_STOP))], track=TRACK)
        with st:
            with pytest.raises(ValueError):
                st.reacquire(**REACQ)
            st.push(f)
            st.flush()
        assert [r for r in gpu_records(phys[0]) if record_tti(r) < tti0 + DRIFT_NSF] == orecs

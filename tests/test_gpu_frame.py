"""Frame sync of a re-acquiring stream on the GPU (lsn_phy_mib_decode_side, lsn_stream_frame_sync): the side PBCH decode against lsn_phy_mib_decode -
also while a submitted block is in flight -, the four cut recordings of frame_cases through a stream - however it is pushed - against the oracle's records and the
figures of the CPU round trip (tests/test_frame_model.py), hold off, no loss, a gap on an attempt's subframe, a check that gives up, status calls in between, and
the refusals that need a device."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import ltesniffer_amd as la
from frame_cases import CUTS, DELTA, EXPECT, NSF, cut_recording, in_force_tti, retagged
from lsn_testlib import TxGen, scenario
from parity import gen_subframes, gpu_records, oracle_records, run_oracle
from reacq_cases import CUT_AFTER, CUT_JUMP_SEGMENT, CUT_PPM
from test_gpu_stream import IRREGULAR, _block, _two_cells
from test_gpu_track import _phys
from track_cases import DRIFT_LEAD, DRIFT_NSF, drifting_recording, record_tti

pytestmark = pytest.mark.gpu
INVALID = -2   # LSN_ERROR_INVALID_INPUTS


# ---- the side decode ----

@pytest.mark.parametrize("over", [{}, dict(cp=1), dict(nof_ports=1, nof_rx=1), dict(nof_ports=4), dict(cp=1, nof_ports=4, snr_db=8.0)])
def test_side_decode_equals_mib_decode(over):
    """25 PRB (N = 512), normal and extended prefix, 1 / 2 / 4 ports, 13 subframes from subframe 8 of SFN 1021 on - two subframes 0 and a subframe 5 among them -:
    the dict and the 480 soft bits of mib_decode_side equal mib_decode's with =="""
    sc = scenario("small", seed=12, start_tti=10 * 1021 + 8, **over)
    tx = TxGen(**sc)
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=4)
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], cp=sc.get("cp", 0))
    found, five = [], 0
    for _ in range(13):
        tti, iq, _ = tx.next()
        side, sllr = phy.mib_decode_side(iq, with_llr=True)
        main, mllr = phy.mib_decode(iq, with_llr=True)
        again = phy.mib_decode_side(iq)
        assert side == main == again and np.array_equal(sllr.view(np.uint32), mllr.view(np.uint32)), (tti, side, main)
        assert side["found"] == (1 if tti % 10 == 0 else 0)
        if side["found"]:
            assert (side["sfn"], side["nof_prb"], side["nof_ports"]) == ((tti // 10) % 1024, sc["nof_prb"], sc["nof_ports"])
            found.append(side["sfn"])
        five += tti % 10 == 5
    assert found == [1022, 1023] and five == 1
    phy.close()


def test_side_decode_while_a_block_is_in_flight():
    """12 subframes submitted with submit_device and not waited for: mib_decode refuses, mib_decode_side gives what mib_decode gave before - on a subframe 0, a
    subframe 5 and a subframe 10 -, and after wait() the block's records are the oracle's"""
    import torch
    sc = scenario("small", seed=7)
    tti0, iq, _ = gen_subframes(sc, 12)
    assert tti0 == 0
    _, _, orecs = run_oracle(sc, tti0, iq, taps=False)
    phy = la.Phy(nof_rx_antennas=sc["nof_rx"], max_batch=12, device=0, pcapwriter=la.PcapWriter(None))
    assert phy.setCell(sc["nof_prb"], sc["nof_ports"], sc["cell_id"])
    before = [phy.mib_decode(iq[i], with_llr=True) for i in (0, 5, 10)]
    assert [b[0]["found"] for b in before] == [1, 0, 1] and before[2][0]["sfn"] == before[0][0]["sfn"] + 1
    d_iq = torch.from_numpy(iq.view(np.float32)).to("cuda:0")
    torch.cuda.synchronize()
    phy.submit_device(d_iq.data_ptr(), 12, tti0)
    with pytest.raises(RuntimeError):
        phy.mib_decode(iq[0])                               # borrows a slot of the pipeline: refused while the block is in flight
    side = [phy.mib_decode_side(iq[i], with_llr=True) for i in (0, 5, 10)]
    phy.wait()
    for (sd, sl), (bd, bl) in zip(side, before):
        assert sd == bd and np.array_equal(sl.view(np.uint32), bl.view(np.uint32))
    assert len(orecs) > 0 and gpu_records(phy) == oracle_records(orecs)
    phy.close()


# ---- the cut recordings through a stream ----

TRACK, REACQ = dict(initial_ppm=CUT_PPM), dict(after=CUT_AFTER)


def _pass(f, sizes, frame_sync, ring_samples=0, block_subframes=16, gap=None, mid=(), reacquire=REACQ):
    """a recording [sample][antenna] through a one-cell Stream -> (count, records, track_status, reacquire_status, frame_sync_status or None).  gap: (lo, hi), the
    samples of the recording that arrive as a declared gap; mid: places at which - behind the first piece that reaches them - the stream is flushed and all three
    statuses are asked"""
    sc, tti0, orecs, opt, rate, _ = drifting_recording()
    with _phys([(sc, opt, None)]) as phys:
        with _block(16):
            st = la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD))], block_subframes=block_subframes, ring_samples=ring_samples, track=TRACK,
                           reacquire=reacquire, frame_sync=frame_sync)
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
                    st.frame_sync_status()
                    seen += 1
            done = st.flush()
            ts, rs = st.track_status(), st.reacquire_status()
            fs = st.frame_sync_status() if frame_sync is not None else None
            assert st.status()["failed"] == 0 and st.status()["samples_pushed"] == len(f)
        return done[0], gpu_records(phys[0]), ts, rs, fs


@functools.lru_cache(maxsize=None)
def _cut_whole(name, hold=True):
    """a cut recording pushed whole with blocks of 16: computed once, shared by the tests below"""
    return _pass(cut_recording(CUTS[name]), (1 << 40,), dict(hold=hold))


def _one(v):
    return {k: x[0] for k, x in v.items()}


@pytest.mark.parametrize("name", list(CUTS))
def test_a_cut_recording_gets_its_tti_back(name):
    """70 001 samples removed, 230 003 removed, 109 000 duplicated, 3000 removed at input sample DRIFT_LEAD + 200 000: the jump at segment 12 lands on the nearest
    PSS, and frame_sync_status is the CPU round trip's - the accepting segment, delta +5 / +25 / -10 / 0, the sfn, the counts.  From T on the records are the
    native stream's, as many as the round trip found, and no record is one the native stream does not have"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    want, native = EXPECT[name], set(orecs)
    n, got, ts, rs, fs = _cut_whole(name)
    print("%s: %d subframes, %d records; track %r; reacquire %r; frame sync %r" % (name, n, len(got), ts, rs, fs))
    assert rs["accepted"] == [1] and rs["last_offset"] == [want["offset"]] and rs["jump_segment"] == [CUT_JUMP_SEGMENT]
    f1 = _one(fs)
    assert (f1["checks"], f1["attempts"], f1["given_up"], f1["accept_segment"], f1["last_delta"], f1["last_sfn"], f1["shift"], f1["held"]) == \
        (1, want["attempts"], 0, want["accept"], DELTA[name], want["sfn"], DELTA[name] % 10240, want["held"])
    assert (f1["relabelled"], f1["confirmed"], f1["relabel_segment"]) == ((1, 0, want["in_force"]) if DELTA[name] else (0, 1, 0))
    T, end = in_force_tti(tti0, f1), tti0 + NSF[name] + DELTA[name]
    assert T == want["T"]
    late = [r for r in orecs if T <= record_tti(r) < end]
    behind = [r for r in got if T <= record_tti(r) < end]
    print("%s: %d of %d native records in [%d, %d), missing TTIs %r" % (name, len(behind), len(late), T, end, sorted(record_tti(r) for r in set(late) - set(behind))))
    assert len(late) == want["late"] and behind == [r for r in late if r in set(behind)] and len(behind) == want["found"]
    assert set(r for r in got if record_tti(r) < tti0 + DRIFT_NSF) <= native                  # hold: none that is not native
    assert len([r for r in got if record_tti(r) < end]) == want["hold"]


def _smallest_ring():
    """the smallest ring lsn_stream_reacquire accepts for blocks of one subframe (test_gpu_reacq.py pins it: 131 072)"""
    sc, tti0, _, opt, rate, _ = drifting_recording()
    ring = 1024
    with _phys([(sc, opt, None)]) as phys:
        while True:
            try:
                with _block(16):
                    la.Stream(rate, [(phys[0], dict(start_tti=tti0, offset_time=DRIFT_LEAD))], block_subframes=1, ring_samples=ring, track=TRACK, reacquire=REACQ,
                              frame_sync={}).close()
                return ring
            except ValueError:
                ring *= 2


@pytest.mark.parametrize("how", ["pieces_1ms", "irregular", "smallest_ring", "blk1", "blk5"])
@pytest.mark.parametrize("name", list(CUTS))
def test_records_and_all_statuses_do_not_depend_on_how_the_stream_is_pushed(name, how):
    """against the cut recording pushed whole with blocks of 16: in 1 ms pieces, in pieces cycling through 1, 7919, 100 003 and 33 samples, through the smallest
    ring lsn_stream_reacquire accepts, with blocks of 1 and 5 subframes - records, track_status, reacquire_status and frame_sync_status equal, the doubles with =="""
    n0, want, ts0, rs0, fs0 = _cut_whole(name)
    kw = dict(pieces_1ms=dict(sizes=(10000,)), irregular=dict(sizes=IRREGULAR), smallest_ring=dict(sizes=(10000,), block_subframes=1),
              blk1=dict(sizes=(1 << 40,), block_subframes=1, ring_samples=1 << 18), blk5=dict(sizes=(1 << 40,), block_subframes=5))[how]
    if how == "smallest_ring":
        kw["ring_samples"] = _smallest_ring()
        assert kw["ring_samples"] == 131072
    n, got, ts, rs, fs = _pass(cut_recording(CUTS[name]), kw.pop("sizes"), dict(), **kw)
    assert n == n0 and got == want
    assert ts == ts0 and rs == rs0 and fs == fs0, (ts, ts0, rs, rs0, fs, fs0)


def test_without_hold_the_subframes_of_the_check_are_written_as_counted():
    """hold off on the recording with 109 000 samples duplicated: what the stream writes more than with hold are the records of segments 12 and 13 - the CPU
    model's 27, each a native record one frame too high -, and everything else, the statuses included, is the same but for the subframes held"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    want, native = EXPECT["duplicated_109000"], set(orecs)
    n0, held, ts0, rs0, fs0 = _cut_whole("duplicated_109000")
    n, got, ts, rs, fs = _cut_whole("duplicated_109000", hold=False)
    extra = [r for r in got if r not in set(held)]
    assert n == n0 and [r for r in got if r in set(held)] == held and len(extra) == want["foreign_nohold"] == want["nohold"] - want["hold"]
    assert all(tti0 + 60 <= record_tti(r) < tti0 + 70 and retagged(r, -10) in native and r not in native for r in extra)
    assert ts == ts0 and rs == rs0 and fs == dict(fs0, held=[0]) and fs0["held"] == [want["held"]]


def test_without_a_loss_nothing_is_checked_and_nothing_changes():
    """frame sync on and nothing lost: the records and the statuses of the same stream without it, zero checks, zero attempts"""
    f = drifting_recording()[5]
    n0, want, ts0, rs0, _ = _pass(f, (1 << 40,), None)
    n, got, ts, rs, fs = _pass(f, (1 << 40,), dict())
    assert n == n0 and got == want and ts == ts0 and rs == rs0
    assert all(v == [0] for v in fs.values()), fs
    assert [r for r in got if record_tti(r) < drifting_recording()[1] + DRIFT_NSF] == drifting_recording()[2]      # every record of the recording


@pytest.mark.parametrize("sizes", [(1 << 40,), (10000,)])
def test_an_attempt_whose_subframe_reads_a_gap_is_not_launched(sizes):
    """109 000 samples duplicated, and 2000 samples inside the first subframe of segment 12 (output subframe 60: input samples 610 034 .. 620 034 behind the lead)
    declared as a gap: that segment has no measurement and its attempt is not launched; the attempt of segment 13 sees a subframe 5, the one of segment 14 decides
    (the one of 15 is in flight then), and the counting is 10 lower from segment 16 on: every native record from TTI 70 on"""
    sc, tti0, orecs, opt, rate, _ = drifting_recording()
    lo = DRIFT_LEAD + 613000
    n, got, ts, rs, fs = _pass(cut_recording(CUTS["duplicated_109000"]), sizes, dict(), gap=(lo, lo + 2000))
    print("gap on the subframe of the first attempt: track %r; reacquire %r; frame sync %r" % (ts, rs, fs))
    whole = _cut_whole("duplicated_109000")
    assert rs == whole[3] and ts["invalid"] == [whole[2]["invalid"][0] + 1]
    assert _one(fs) == dict(_one(whole[4]), attempts=3, accept_segment=14, relabel_segment=16, last_sfn=EXPECT["duplicated_109000"]["sfn"] + 1, held=20)
    end = tti0 + NSF["duplicated_109000"] - 10
    assert [r for r in got if tti0 + 70 <= record_tti(r) < end] == [r for r in orecs if tti0 + 70 <= record_tti(r) < end]
    assert set(r for r in got if record_tti(r) < tti0 + DRIFT_NSF) <= set(orecs) and not [r for r in got if tti0 + 50 <= record_tti(r) < tti0 + 70]


def test_a_check_that_runs_out_of_tries_gives_up_and_leaves_the_tti():
    """tries = 1 on the recording with 70 001 samples removed: the one attempt lands on a subframe 5.  given_up 1, no shift, segments 12 and 13 held - and the
    records are those of the stream without frame sync: the counting stays a half frame off and nothing behind the cut decodes"""
    n, got, ts, rs, fs = _pass(cut_recording(CUTS["removed_70001"]), (1 << 40,), dict(tries=1))
    n0, want, ts0, rs0, _ = _pass(cut_recording(CUTS["removed_70001"]), (1 << 40,), None)
    assert _one(fs) == dict(checks=1, attempts=1, confirmed=0, relabelled=0, given_up=1, accept_segment=0, relabel_segment=0, held=10, last_sfn=0, last_delta=0, shift=0)
    assert n == n0 and got == want and ts == ts0 and rs == rs0 and len(got) == EXPECT["removed_70001"]["off"]


def test_flushes_and_status_calls_in_between_change_nothing():
    """a flush and all three status calls every 3 ms from in front of the jump (segment 12 begins near input sample 511 000) to behind the segment the relabel
    takes force at (15, near 661 000): they fetch measurements, the search's result and the attempts early, and records and statuses at the end are still those
    of the recording pushed whole"""
    n0, want, ts0, rs0, fs0 = _cut_whole("removed_70001")
    mid = tuple(DRIFT_LEAD + 440000 + 30000 * i + 4321 for i in range(10))
    n, got, ts, rs, fs = _pass(cut_recording(CUTS["removed_70001"]), (10000,), dict(), mid=mid)
    assert n == n0 and got == want and ts == ts0 and rs == rs0 and fs == fs0, (ts, ts0, rs, rs0, fs, fs0)


def test_without_frame_sync_the_recording_stays_half_a_frame_off():
    """what the feature is for: 70 001 samples removed through a stream that re-acquires and does not check - the jump lands on the nearest PSS, a half frame off,
    and no record behind the cut is found"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    n, got, ts, rs, _ = _pass(cut_recording(CUTS["removed_70001"]), (1 << 40,), None)
    assert rs["accepted"] == [1] and rs["jump_segment"] == [CUT_JUMP_SEGMENT] and ts["lost"] == [0]
    assert not [r for r in got if record_tti(r) >= tti0 + 5 * CUT_JUMP_SEGMENT] and len(got) == EXPECT["removed_70001"]["off"] and set(got) <= set(orecs)


# ---- refusals ----

def test_refusals_leave_the_stream_usable():
    cells, orecs, rate_in, raw, scale, _ = _two_cells(la.FILE_CF32)

    def stream(phys, **kw):
        with _block(16):
            return la.Stream(rate_in, [(p, k) for p, (_, _, k) in zip(phys, cells)], block_subframes=1, ring_samples=1 << 20, **kw)
    with _phys(cells) as phys:
        with stream(phys) as st:
            with pytest.raises(ValueError):
                st.frame_sync()                                                  # an untracked stream
            with pytest.raises(ValueError):
                st.frame_sync_status()
            st.track()
            with pytest.raises(ValueError):
                st.frame_sync()                                                  # tracked, without lsn_stream_reacquire
            st.reacquire()
            cfg = la._frame_sync_cfg(2)
            cfg.struct_size += 4
            assert la.lib().lsn_stream_frame_sync(st._h, C.byref(cfg)) == INVALID # a size-off struct_size
            cfg = la._frame_sync_cfg(2)
            cfg.hold = 3
            assert la.lib().lsn_stream_frame_sync(st._h, C.byref(cfg)) == INVALID # a hold it does not know
            with pytest.raises(ValueError):
                st.frame_sync(tries=65)
            with pytest.raises(ValueError):
                st.frame_sync(enable=[True])
            with pytest.raises(ValueError):
                st.frame_sync_status()                                           # no frame sync
            st.push(raw[:1000])
            with pytest.raises(ValueError):
                st.frame_sync()                                                  # after a push
            st.push(raw[1000:])
            assert st.flush() == [12, 12]
        assert [gpu_records(p) for p in phys] == orecs
    # accepted - tries = 64 is -, one call only, and twelve subframes with nothing lost: no check, the oracle's records
    with _phys(cells) as phys:
        with stream(phys, track=dict(), reacquire=dict(after=1), frame_sync=dict(tries=64, enable=[True, False])) as st:
            with pytest.raises(ValueError):
                st.frame_sync()
            st.push(raw)
            assert st.flush() == [12, 12]
            fs = st.frame_sync_status()
            assert fs["checks"] == [0, 0] and fs["attempts"] == [0, 0] and fs["held"] == [0, 0]
        assert [gpu_records(p) for p in phys] == orecs

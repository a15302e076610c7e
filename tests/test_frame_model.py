"""Frame sync of a re-acquiring stream without a GPU (lsn_frame_sync_decide, the rule of DESIGN 3.1m): the library's decision against the Python model with ==,
the rule as a state machine, the round trip of four cut recordings through the model loop, the rule and the oracle - with hold, without it and with the rule off -,
the slip by exactly two half frames that nothing notices, and the refusals that need no device."""
import ctypes as C

import pytest

import frame_model as fm
import ltesniffer_amd as la
from frame_cases import CUTS, DELTA, EXPECT, NSF, SILENT, in_force_tti, oracle_at, replay, retagged, round_trip
from reacq_cases import CUT_JUMP_SEGMENT, CUT_SEARCH_SEGMENT
from track_cases import DRIFT_NSF, drifting_recording, record_tti

INVALID = -2   # LSN_ERROR_INVALID_INPUTS


# ---- 1. the library's decision against the model: equal ----

def _mib(sfn, nof_prb=25, nof_ports=2, found=1):
    return dict(found=found, sfn=sfn, nof_prb=nof_prb, nof_ports=nof_ports)


def test_decision_of_the_library_is_the_models():
    counted = (0, 5, 10, 2555, 5110, 5115, 5120, 5125, 5130, 10225, 10230, 10235)
    sfns = (0, 1, 2, 255, 510, 511, 512, 513, 514, 1022, 1023)
    seen = set()
    for c in counted:                                       # every wrap of C and T around 10240, sfn 0 and 1023
        for sfn in sfns:
            want = fm.decide(_mib(sfn), 25, 2, c)
            assert la.frame_sync_decide(_mib(sfn), 25, 2, c) == want, (c, sfn)
            assert want[0] and -5120 < want[1] <= 5120 and want[1] % 5 == 0 and (c + want[1]) % 10240 == 10 * sfn
            seen.add(want[1])
    assert {0, 5, -5, 10, -10, 5120, 5115, -5115} <= seen   # (-5120 does not exist: the half turn counts as +5120)
    assert la.frame_sync_decide(_mib(512), 25, 2, 0) == (True, 5120) and la.frame_sync_decide(_mib(0), 25, 2, 5120) == (True, 5120)
    assert la.frame_sync_decide(_mib(0), 25, 2, 5125) == (True, 5115) and la.frame_sync_decide(_mib(0), 25, 2, 5115) == (True, -5115)
    # each mismatch: not found, another bandwidth, another number of ports - whatever C is
    for bad in (None, _mib(7, found=0), _mib(7, nof_prb=50), _mib(7, nof_prb=6), _mib(7, nof_ports=1), _mib(7, nof_ports=4)):
        for c in (65, 66, 0):
            assert la.frame_sync_decide(bad, 25, 2, c) == fm.decide(bad, 25, 2, c) == (False, 0)
    assert la.frame_sync_decide(_mib(7, nof_prb=100, nof_ports=4), 100, 4, 65) == (True, 5)
    # an accepted MIB on a segment that does not begin on a multiple of 5: an internal error, not a case
    for c in (1, 64, 10239):
        with pytest.raises(RuntimeError):
            la.frame_sync_decide(_mib(7), 25, 2, c)
        with pytest.raises(AssertionError):
            fm.decide(_mib(7), 25, 2, c)


# ---- 2. the rule as a state machine ----

def _run(rule, segments, jumps, results, gaps=()):
    """-> per segment (first TTI, holding), the attempts that were looked at"""
    asked, out = [], []

    def result(a):
        asked.append(a)
        return results.get(a)
    for h in range(segments):
        rule.entered(h, h in jumps, result)
        rule.launched(h, h in gaps)
        out.append((rule.tti(5 * h), rule.holding))
    return out, asked


def test_rule_attempts_every_segment_and_takes_a_result_in_two_segments_later():
    """a jump at segment 12 whose first subframe is a subframe 5: the attempt of 12 finds nothing, the one of 13 (counted 65) decodes sfn 7.  It is looked at on
    entering 15 and the TTI is 5 higher from there; the attempt of 14 was in flight then and is dropped; segments 12 .. 14 are held"""
    rule = fm.Rule(25, 2)
    out, asked = _run(rule, 20, {12}, {13: _mib(7), 14: _mib(99)})
    assert asked == [12, 13]
    assert [t for t, _ in out] == [5 * h for h in range(15)] + [5 * h + 5 for h in range(15, 20)]
    assert [h for h, (_, held) in enumerate(out) if held] == [12, 13, 14]
    assert rule.status == dict(checks=1, attempts=3, confirmed=0, relabelled=1, given_up=0, accept_segment=13, relabel_segment=15, last_sfn=7, last_delta=5, shift=5)
    # without hold nothing is held and everything else is the same
    rule2 = fm.Rule(25, 2, hold=False)
    out2, _ = _run(rule2, 20, {12}, {13: _mib(7)})
    assert [t for t, _ in out2] == [t for t, _ in out] and not any(held for _, held in out2) and rule2.status == rule.status
    # a confirmation: delta 0 ends the check and changes no TTI
    rule3 = fm.Rule(25, 2)
    out3, _ = _run(rule3, 20, {12}, {12: _mib(6)})
    assert [t for t, _ in out3] == [5 * h for h in range(20)] and [h for h, (_, held) in enumerate(out3) if held] == [12, 13]
    assert rule3.status["confirmed"] == 1 and rule3.status["relabelled"] == 0 and rule3.status["relabel_segment"] == 0 and rule3.status["attempts"] == 2


def test_rule_a_second_jump_restarts_the_check():
    """jumps at 12 and 13: the attempt of 12 comes back on entering 14, in front of the running check's first segment, and is ignored - even though it decodes"""
    rule = fm.Rule(25, 2)
    out, asked = _run(rule, 20, {12, 13}, {12: _mib(500), 14: _mib(9)})
    assert asked == [13, 14] and rule.status["checks"] == 2 and rule.status["accept_segment"] == 14 and rule.status["last_delta"] == 20
    assert [h for h, (_, held) in enumerate(out) if held] == [12, 13, 14, 15] and out[16][0] == 100
    # a jump at the very segment a decision takes force at: the decision first, then the new check
    rule = fm.Rule(25, 2)
    out, asked = _run(rule, 20, {12, 14}, {12: _mib(7), 14: _mib(8)})
    assert out[14] == (80, True) and rule.status["checks"] == 2 and rule.status["relabelled"] == 1 and rule.status["confirmed"] == 1 and rule.status["shift"] == 10


def test_rule_a_gap_on_the_attempts_subframe_counts_as_not_found():
    rule = fm.Rule(25, 2)
    out, asked = _run(rule, 20, {12}, {12: _mib(6), 13: _mib(7), 14: _mib(8)}, gaps={12})
    assert asked == [13] and rule.status["attempts"] == 2 and rule.status["accept_segment"] == 13 and rule.status["last_delta"] == 5 and out[15] == (80, False)


def test_rule_gives_up_after_tries_attempts():
    rule = fm.Rule(25, 2, tries=2)
    out, asked = _run(rule, 20, {12}, {14: _mib(3)})
    assert asked == [12, 13] and rule.status["attempts"] == 2 and rule.status["given_up"] == 1 and rule.status["shift"] == 0
    assert [h for h, (_, held) in enumerate(out) if held] == [12, 13, 14] and [t for t, _ in out] == [5 * h for h in range(20)]
    rule = fm.Rule(25, 2)                                   # the default: 8
    out, asked = _run(rule, 30, {12}, {})
    assert asked == list(range(12, 20)) and rule.status["given_up"] == 1 and [h for h, (_, held) in enumerate(out) if held] == list(range(12, 21))


# ---- 3. the round trip ----

@pytest.mark.parametrize("name", list(CUTS))
def test_round_trip_of_a_cut_recording(name):
    """the drifting recording cut at input sample DRIFT_LEAD + 200 000 - 70 001 samples removed, 230 003 removed, 109 000 duplicated, 3000 removed - through the model
    loop and the rule of 3.1k (one search at segment 9, the jump in force at 12, the nearest PSS) and then the rule of 3.1m, fed by the oracle's PBCH decode of the
    first subframes of segments 12 ...: delta +5, +25, -10, 0.  The oracle worker at the TTIs the rule assigns finds, from T on, the native stream's records -
    all of them but for the 23 ms cut, where 11 of 777 are missing: those of TTI 100 .. 103, the FIRST four subframes of the new counting (segment 15), not the
    last of the shortened recording - and with hold none that no native subframe has.  With the rule off and delta != 0 it finds none of them: today's stream"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    native, want = set(orecs), EXPECT[name]
    r = round_trip(name)
    st = r["status"]
    T = in_force_tti(tti0, st)
    end = tti0 + NSF[name] + DELTA[name]
    late = [x for x in orecs if T <= record_tti(x) < end]
    figures = {}
    for mode, rr in (("hold", r), ("nohold", round_trip(name, hold=False)), ("off", round_trip(name, rule=False))):
        got = rr["records"]
        figures[mode] = (len(got), len([x for x in got if x in native and record_tti(x) >= T]), len([x for x in got if x not in native]))
    missing = sorted(record_tti(x) for x in set(late) - set(r["records"]))
    print("%s: searches %r, jumps %r, status %r, attempts looked at %r, T %d, %d native records in [T, %d); (records, native from T on, not native): %r; missing TTIs %r" %
          (name, r["searches"], r["jumps"], st, r["asked"], T, len(late), end, figures, missing))
    assert [(s[0], s[1], s[2]) for s in r["searches"]] == [(CUT_SEARCH_SEGMENT, True, want["offset"])] and r["jumps"] == [(CUT_JUMP_SEGMENT, want["offset"])]
    assert st["checks"] == 1 and st["accept_segment"] == want["accept"] and st["last_delta"] == DELTA[name] and st["last_sfn"] == want["sfn"] and T == want["T"]
    assert st["shift"] == DELTA[name] % 10240 and st["given_up"] == 0 and st["attempts"] == want["attempts"] and st["held"] == want["held"]
    assert (st["relabelled"], st["confirmed"], st["relabel_segment"]) == ((1, 0, want["in_force"]) if DELTA[name] else (0, 1, 0))
    assert want["in_force"] == want["accept"] + 2 and r["asked"] == list(range(CUT_JUMP_SEGMENT, want["accept"] + 1))
    assert len(late) == want["late"]
    assert figures["hold"] == (want["hold"], want["found"], 0)                                  # with hold: no record that is not native
    assert figures["nohold"] == (want["nohold"], want["found"], want["foreign_nohold"])
    assert figures["off"] == (want["off"], want["found"] if not DELTA[name] else 0, want["foreign_off"])      # the rule off and delta != 0: no native record from T on
    assert [x for x in r["records"] if record_tti(x) >= T] == [x for x in late if x in set(r["records"])] and len(missing) == want["late"] - want["found"]
    if name == "removed_230003":
        assert missing == [100, 100, 100, 101, 101, 101, 102, 102, 103, 103, 103]
    # what hold keeps back is what the stream without it writes with the old counting between the jump and the decision
    extra = [x for x in round_trip(name, hold=False)["records"] if x not in set(r["records"])]
    assert len(extra) == want["nohold"] - want["hold"] and all(tti0 + 5 * CUT_JUMP_SEGMENT <= record_tti(x) < tti0 + 5 * want["in_force"] for x in extra)
    if name == "duplicated_109000":                         # a slip by two half frames decodes, every record one frame too high
        assert all(retagged(x, -10) in native for x in extra) and len(extra) == want["foreign_nohold"]


def test_a_slip_by_exactly_two_half_frames_is_silent():
    """exactly 100 000 samples duplicated: no PSS moves, nothing is searched, nothing is checked - and every record behind the slip is 10 TTIs too high"""
    sc, tti0, orecs, opt, rate, f = drifting_recording()
    iq, log, searches, jumps = replay(SILENT, DRIFT_NSF)
    assert not searches and not jumps and max(run for _, _, run in log) <= 1
    got = oracle_at(sc, opt, iq, [tti0 + i for i in range(DRIFT_NSF)], [False] * DRIFT_NSF)
    native = set(orecs)
    behind = [x for x in got if record_tti(x) >= tti0 + 30]
    print("100 000 samples duplicated: %d records, %d of them from TTI %d on, of which %d are native as written and %d one frame earlier" %
          (len(got), len(behind), tti0 + 30, len([x for x in behind if x in native]), len([x for x in behind if retagged(x, -10) in native])))
    assert len(behind) > 800 and not any(x in native for x in behind) and all(retagged(x, -10) in native for x in behind)


# ---- 4. refusals that need no device ----

def test_refusals_without_a_device():
    L = la.lib()
    cfg = la._frame_sync_cfg(0)
    assert L.lsn_stream_frame_sync(None, C.byref(cfg)) == INVALID and L.lsn_stream_frame_sync(None, None) == INVALID      # no stream
    status = la.StreamFrameSyncStatus()
    status.struct_size = C.sizeof(status)
    assert L.lsn_stream_frame_sync_status(None, C.byref(status)) == INVALID
    m = la.Mib()
    assert L.lsn_phy_mib_decode_side(None, None, 0, C.byref(m), None) == INVALID
    with pytest.raises(ValueError):
        la._frame_sync_cfg(2, enable=[True])
    assert la._frame_sync_cfg(1).hold == 1 and la._frame_sync_cfg(1, hold=False).hold == la.FRAME_SYNC_NO_HOLD == 2 and la._frame_sync_cfg(1, hold=0).hold == 2
    # the sizes the header states
    assert C.sizeof(la.StreamFrameSyncCfg) == 12 + 4 * 8 and C.sizeof(la.StreamFrameSyncStatus) == 8 + 8 * 64 + 3 * 32
    d = C.c_int32()
    assert L.lsn_frame_sync_decide(None, 25, 2, 0, C.byref(d)) == INVALID and L.lsn_frame_sync_decide(C.byref(m), 25, 2, 0, None) == INVALID
    for bad in (10240, 10245, 1 << 31):
        with pytest.raises(ValueError):
            la.frame_sync_decide(_mib(7), 25, 2, bad)
    with pytest.raises(ValueError):
        la.frame_sync_decide(_mib(1024), 25, 2, 0)

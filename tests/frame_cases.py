"""Inputs of the frame-sync tests (CPU and GPU): the drifting recording of track_cases cut so far that re-acquisition lands on another half frame - or, cut by whole
half frames, finds nothing to do -, and the float64 round trip: reacq_cases.model_replay, the rule of DESIGN 3.1m (frame_model.Rule) fed by the oracle's PBCH decode
of the replayed subframes, and the oracle worker run at the TTIs the rule assigns."""
import functools

import numpy as np

import frame_model as fm
from reacq_cases import CUT_AFTER, CUT_AT, CUT_PPM, model_replay
from track_cases import DRIFT_NSF, drifting_recording, record_tti

# samples removed (negative) or duplicated (positive) at CUT_AT, and the subframes the cut recording still replays in full: 7 ms and 23 ms removed end that much
# earlier, less the 2 ms the jump moves the position back or forth
CUTS = {"removed_70001": -70001, "removed_230003": -230003, "duplicated_109000": 109000, "removed_3000": -3000}
NSF = {"removed_70001": 395, "removed_230003": 375, "duplicated_109000": DRIFT_NSF, "removed_3000": DRIFT_NSF}
# what the issue expects of them: the shift in subframes
DELTA = {"removed_70001": 5, "removed_230003": 25, "duplicated_109000": -10, "removed_3000": 0}
SILENT = 100000          # duplicated: exactly 10 ms, no PSS moves
# what the CPU round trip gives (tests/test_frame_model.py recomputes and asserts every figure; the GPU tests compare a stream against them).  All four: one search,
# at segment 9, the jump in force at segment 12.  offset: the search's, output samples; accept: the segment whose attempt is accepted; in_force: the segment from
# which the decision holds; T: the TTI of that segment's first subframe; attempts launched; held subframes; late: the oracle's records of the native stream with
# T <= TTI < the end of the replay; found: those of them the round trip finds (with and without hold); records with hold, without it, and with the rule off;
# foreign: records no native subframe has, without hold and with the rule off (with hold: none)
EXPECT = {
    "removed_70001": dict(offset=-15356, accept=13, in_force=15, sfn=7, T=80, attempts=3, held=15, late=832, found=832, hold=883, nohold=883, off=51, foreign_nohold=0, foreign_off=0),
    "removed_230003": dict(offset=15368, accept=13, in_force=15, sfn=9, T=100, attempts=3, held=15, late=777, found=766, hold=817, nohold=817, off=51, foreign_nohold=0, foreign_off=0),
    "duplicated_109000": dict(offset=6908, accept=12, in_force=14, sfn=5, T=60, attempts=2, held=10, late=857, found=857, hold=908, nohold=935, off=935, foreign_nohold=27, foreign_off=884),
    "removed_3000": dict(offset=-2304, accept=12, in_force=14, sfn=6, T=70, attempts=2, held=10, late=856, found=856, hold=907, nohold=933, off=933, foreign_nohold=0, foreign_off=0),
}


def in_force_tti(tti0, status):
    """T: the TTI of the first subframe of the segment from which the accepted attempt's decision holds"""
    return (tti0 + 5 * (status["accept_segment"] + fm.DELAY) + status["shift"]) % fm.WRAP


@functools.lru_cache(maxsize=None)
def cut_recording(n):
    """the drifting recording [sample][antenna] complex64 with n samples removed (n < 0) or duplicated (n > 0) at CUT_AT, read-only"""
    f = drifting_recording()[5]
    g = np.concatenate([f[:CUT_AT], f[CUT_AT - n:]] if n < 0 else [f[:CUT_AT], f[CUT_AT - n:CUT_AT], f[CUT_AT:]])
    g.setflags(write=False)
    return g


def mib_of(sc, iq):
    """the oracle's PBCH decode of one subframe [antenna][15 N] -> the dict of Phy.mib_decode, or None"""
    from test_pbch_oracle import oracle_mib
    r, m = oracle_mib(sc, iq)
    return dict(found=1, sfn=int(m.sfn), nof_prb=int(m.nof_prb), nof_ports=int(m.nof_ports)) if r == 1 else None


def run_rule(sc, tti0, iq, jumps, tries=0, hold=True, gaps=()):
    """the rule over the segments of a replay.  iq [nsf][antenna][15 N], jumps [(segment in force, o)], gaps: segments whose first subframe reads a declared gap
    -> (per-subframe TTI, per-subframe held, the rule's status, the segments whose attempt was asked for)"""
    rule = fm.Rule(sc["nof_prb"], sc["nof_ports"], tti0, tries, hold)
    asked = []

    def result(a):
        asked.append(a)
        return mib_of(sc, iq[5 * a])
    tti, held = [], []
    at = set(h for h, _ in jumps)
    for h in range(len(iq) // 5):
        rule.entered(h, h in at, result)
        rule.launched(h, h in gaps)
        tti += [rule.tti(sf) for sf in range(5 * h, 5 * h + 5)]
        held += [rule.holding] * 5
    return tti, held, dict(rule.status, held=sum(held)), sorted(set(asked))


def oracle_at(sc, opt, iq, tti, held):
    """the oracle worker over the subframes that are not held, each at its TTI -> records"""
    from lsn_testlib import OracleWorker, oracle_trace_enable, parse_pcap
    from parity import oracle_records
    oracle_trace_enable(False)
    ow = OracleWorker(sc["nof_prb"], sc["nof_ports"], sc["cell_id"], sc["nof_rx"], sc["phich_ng_x6"], **dict(dict(cp=sc.get("cp", 0)), **opt))
    for i in range(len(iq)):
        if not held[i]:
            ow.work(iq[i], tti[i])
    return oracle_records(parse_pcap(ow.pcap_bytes()))


@functools.lru_cache(maxsize=None)
def replay(n, nsf):
    """reacq_cases.model_replay of a cut recording with the stream's settings of the tests (initial_ppm = 60, after = 4), computed once"""
    rate = drifting_recording()[4]
    return model_replay(cut_recording(n), rate, nsf, initial_ppm=CUT_PPM, after=CUT_AFTER)


@functools.lru_cache(maxsize=None)
def round_trip(name, hold=True, tries=0, gaps=(), rule=True):
    """-> dict(searches, jumps, status, tti, held, asked, records); rule False: today's stream, every subframe as counted"""
    sc, tti0, _, opt, _, _ = drifting_recording()
    iq, _, searches, jumps = replay(CUTS[name], NSF[name])
    if rule:
        tti, held, status, asked = run_rule(sc, tti0, iq, jumps, tries, hold, gaps)
    else:
        tti, held, status, asked = [(tti0 + i) % fm.WRAP for i in range(len(iq))], [False] * len(iq), None, []
    return dict(searches=searches, jumps=jumps, status=status, tti=tti, held=held, asked=asked, records=oracle_at(sc, opt, iq, tti, held))


def retagged(rec, delta):
    """a MAC-LTE record with its TTI moved by delta subframes (track_cases.record_tti's two bytes)"""
    t = (record_tti(rec) + delta) % fm.WRAP
    fs = ((t // 10) << 4) | (t % 10)
    return rec[:10] + bytes([fs >> 8, fs & 255]) + rec[12:]

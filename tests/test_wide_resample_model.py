"""The resampler's wide-ratio range (4 < rate_in / rate_out <= 32: DESIGN 3.1b "accepted range", 3.1o), without a GPU: what is accepted and with how many taps,
the run geometry against the rule in Python integers (the C++ side is tests/native/test_resample_geometry.cc, a program of its own built with
-fsanitize=address,undefined), the filter's quality on exact tones through the float64 model of tests/wide_resample_model.py, the plans of a file pass and of a
stream over a recording with a narrow cell, and the round trips model -> complex64 -> CPU oracle that license the GPU record tests of test_gpu_wide_resample.py.

Output rates below 3.84 MS/s stay refused above ratio 4 (the 6-PRB cell's 1.92 MS/s: tests/test_scan_model.py asserts those refusals), so the 6-PRB rows of the
rate tables are asserted REFUSED here, the 6-PRB round trip does not exist, and the tones at ratios 16 and 32 are a 15-PRB cell's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ltesniffer_amd as la
import resample_cases
from lsn_testlib import ROOT
from resample_cases import LEAD, check_tones
from resample_model import Plan, passband_hz
from wide_resample_model import SYMBOL_SZ, WIDE_NSF, WIDE_RATE, WidePlan, accepted, geometry, wide_recording

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
PPM = 150e-6
RATES_IN = (122.88e6, 122.88e6 * (1 - PPM), 61.44e6)
TABLE = sorted({(prb, 15000.0 * N) for tab in SYMBOL_SZ for prb, N in tab.items()})     # every (nof_prb, rate) of both rate tables


def _taps(rate_in, rate_out, B):
    cfg = la._resample_cfg(1, rate_in, rate_out, 0, 0.0, 0, 0, B, la.FILE_CF32, 0.0)
    sp = la.ResampleSpan()
    rc = la.lib().lsn_resample_span(C.byref(cfg), 0, 10 ** 9, C.byref(sp))
    assert rc in (0, INVALID)
    return int(sp.taps) if rc == 0 else None


def test_accepted_table():
    """every (bandwidth, rate table) pair at or above 3.84 MS/s from 122.88, 122.88 (1 - 150 ppm) and 61.44 MS/s: accepted with the model's taps, at most 768"""
    worst = 0
    for rate_in in RATES_IN:
        for prb, rate_out in TABLE:
            B = passband_hz(prb)
            got = _taps(rate_in, rate_out, B)
            if rate_out < 3.84e6 and rate_in > 4 * rate_out:
                assert got is None and not accepted(rate_in, rate_out, B), (rate_in, prb)      # the 6-PRB cell above ratio 4: refused as before
                continue
            plan = WidePlan(rate_in, rate_out, B)
            assert got == plan.taps <= 768, (rate_in, prb, rate_out, got, plan.taps)
            worst = max(worst, got)
    assert worst == WidePlan(122.88e6, 3.84e6, passband_hz(15)).taps == 558
    assert _taps(122.88e6, 5.76e6, passband_hz(25)) == 504 and _taps(122.88e6, 15.36e6, passband_hz(75)) == 338 and _taps(122.88e6, 7.68e6, passband_hz(25)) == 198
    # the ceilings: rate_in above 122.88 MS/s, ratio above 32, and an estimate above 768 taps
    assert _taps(122.88e6 + 1.0, 7.68e6, passband_hz(25)) is None and _taps(123e6, 30.72e6, passband_hz(100)) is None
    assert _taps(122.88e6, 3.84e6 - 1.0, passband_hz(15)) is None                       # ratio just above 32 = an output rate below 3.84 MS/s
    assert _taps(122.88e6, 122.88e6 / 65, 0.3e6) is None and _taps(122.88e6, 1.92e6, passband_hz(6)) is None
    assert _taps(122.88e6, 3.84e6, 1.75e6) is None and not accepted(122.88e6, 3.84e6, 1.75e6)     # width 0.00277: 1813 taps
    # ratios up to 4 report what they reported: Plan is the model with the old range
    for rate_in, rate_out, prb in resample_cases.PAIRS + [(30.72e6, 7.68e6, 25), (7.68e6, 1.92e6, 6)]:
        old = Plan(rate_in, rate_out, passband_hz(prb))
        assert _taps(rate_in, rate_out, passband_hz(prb)) == old.taps == WidePlan(rate_in, rate_out, passband_hz(prb)).taps <= 192
    assert _taps(30.72e6, 30.72e6, 14.97e6) is None                                       # more than 192 taps at ratio 1 stays refused


def test_geometry_equals_the_rule_in_python_integers():
    """lanes per output, outputs per run and staged samples per run of the library (header-only C++ under the sanitizers) against wide_resample_model.geometry, for
    every accepted row of the table, steps on both sides of every boundary of the rule, and a tracked segment's widened step; span * 8 <= 64 KiB everywhere"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "native"), "-f", "wide_resample.mk", "_build/test_resample_geometry"], stdout=subprocess.DEVNULL)
    rows = []
    for rate_in in RATES_IN + (30.75e6,):
        for prb, rate_out in TABLE:
            if accepted(rate_in, rate_out, passband_hz(prb)):
                p = WidePlan(rate_in, rate_out, passband_hz(prb))
                rows.append((p.step, p.step + (p.step * 120) // 10 ** 6, p.taps))           # a segment 120 ppm fast, the tracker's limit
    for k in (4, 8, 16, 32):
        rows += [((k << 64) - 1, (k << 64) + 5, 768), (k << 64, k << 64, 764), ((k << 64) + 1, (k << 64) - 5, 200)]
    rows += [(1 << 63, 1 << 63, 50), ((1 << 64) + 12345, 1 << 64, 192)]
    args = []
    for step, seg, taps in rows:
        args += ["%x" % (step >> 64), "%x" % (step & (2 ** 64 - 1)), "%x" % (seg >> 64), "%x" % (seg & (2 ** 64 - 1)), str(taps)]
    out = subprocess.check_output([os.path.join(ROOT, "tests", "native", "_build", "test_resample_geometry")] + args).decode().split("\n")
    got = [tuple(int(w) for w in line.split()) for line in out if line.strip()]
    assert len(got) == len(rows)
    seen = set()
    for (step, seg, taps), (grp, run, span, seg_span) in zip(rows, got):
        g, r, s = geometry(step, taps)
        assert (grp, run, span) == (g, r, s) and seg_span == ((r * seg) >> 64) + taps + 2, (hex(step), taps, grp, run, span, seg_span)
        assert span * 8 <= 65536 and seg_span * 8 <= 65536 and (grp == 0 or (grp >= 8 and (grp << 64) >= min(step, 32 << 64) and run * grp == 4096))
        seen.add(grp)
    assert seen == {0, 8, 16, 32}


# (rate_in, rate_out, nof_prb, outputs): ratios 8, 10.67, 16 and 32 - the 15-PRB pairs stand where a 6-PRB pair would, had 1.92 MS/s outputs not stayed refused;
# fewer outputs where the filter is long (the cost is outputs x taps x tones)
TONE_PAIRS = [(61.44e6, 7.68e6, 25, 3000), (61.44e6, 5.76e6, 25, 2000), (61.44e6, 3.84e6, 15, 1500), (122.88e6, 3.84e6, 15, 1000)]


@pytest.mark.parametrize("rate_in,rate_out,nof_prb,n_out", TONE_PAIRS)
def test_model_meets_the_quality_requirement_on_exact_tones(rate_in, rate_out, nof_prb, n_out, monkeypatch):
    monkeypatch.setattr(resample_cases, "Plan", WidePlan)     # check_tones builds its plan: the wide range's
    worst_pass, worst_land = check_tones(lambda plan, x, in_base, n_out: plan.apply(x, 0, n_out, in_base=in_base), rate_in, rate_out, nof_prb, n_out=n_out)
    print("wide model %.2f -> %.2f MS/s, %d PRB: pass band %.1f dB, landing in band %.1f dB" %
          (rate_in / 1e6, rate_out / 1e6, nof_prb, 20 * np.log10(worst_pass), 20 * np.log10(max(worst_land, 1e-30))))
    assert worst_pass <= 1e-3 and worst_land <= 1e-3, (worst_pass, worst_land)


def _placed(cells, **kw):
    return [dict(nof_prb=sc["nof_prb"], center_offset_hz=f0, offset_time=LEAD, max_subframes=WIDE_NSF, **kw) for sc, _, _, _, f0, _ in cells]


def test_plans_of_a_file_pass_and_a_stream_over_the_recording_are_the_models():
    cells, f = wide_recording()
    placed = _placed(cells)
    plans = [WidePlan(WIDE_RATE, native, passband_hz(sc["nof_prb"]), LEAD, 0.0) for sc, _, _, _, _, native in cells]
    assert [p.grp for p in plans] == [0, 8] and [p.taps for p in plans] == [_taps(WIDE_RATE, p.rate_out, passband_hz(sc[0]["nof_prb"])) for p, sc in zip(plans, cells)]
    done = [0, 0]
    for k in range(100):
        b = la.file_cells_span(WIDE_RATE, placed, len(f), block=k, blk_subframes=5, nof_antennas=2)
        if not b["nof_active"]:
            break
        assert b["taps"] == [p.taps for p in plans] and b["first_subframe"] == done
        spans = [p.span(sf0 * int(p.rate_out) // 1000, n * int(p.rate_out) // 1000) for p, sf0, n in zip(plans, b["first_subframe"], b["nof_subframes"]) if n]
        assert (b["in_lo"], b["in_hi"]) == (max(min(s[0] for s in spans), 0), max(s[1] for s in spans)) and b["in_hi"] <= len(f)
        done = [d + n for d, n in zip(done, b["nof_subframes"])]
    assert done == [WIDE_NSF, WIDE_NSF]
    for blk in (1, 4):
        s = la.stream_span(WIDE_RATE, placed, 0, nof_antennas=2, block_subframes=blk)
        spans = [p.span(0, blk * int(p.rate_out) // 1000) for p in plans]
        assert s["taps"] == [p.taps for p in plans] and s["block_input"] == max(x[1] for x in spans) - min(x[0] for x in spans) + 2
    # the whole recording pushed: every subframe of both cells is complete
    assert la.stream_span(WIDE_RATE, placed, len(f), nof_antennas=2, block_subframes=1)["subframes_complete"][:2] == [WIDE_NSF, WIDE_NSF]
    # a 15-PRB cell at ratio 32 in the default block buffer of 800 subframes: the block shrinks to what fits, at least one subframe
    b = la.file_cells_span(122.88e6, [dict(nof_prb=15, offset_time=LEAD)], 122880 * 40, nof_antennas=1)
    wide = WidePlan(122.88e6, 3.84e6, passband_hz(15), LEAD, 0.0)
    assert 1 <= b["blk_used"] <= 800 * 3840 // 122880 and b["taps"] == [wide.taps] and (b["in_lo"], b["in_hi"]) == wide.span(0, b["blk_used"] * 3840)
    with pytest.raises(ValueError):     # the 6-PRB cell at ratio 64 stays refused
        la.file_cells_span(122.88e6, [dict(nof_prb=6, offset_time=LEAD)], 122880 * 40, nof_antennas=1)


def _decode(sc, tti0, opt, y, nant, sflen):
    from lsn_testlib import oracle_trace
    from parity import oracle_records, run_oracle
    iq = np.ascontiguousarray(y.reshape(WIDE_NSF, sflen, nant).transpose(0, 2, 1)).astype(np.complex64)
    _, _, recs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
    return oracle_records(recs), oracle_trace()


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_round_trip_of_the_recording_through_the_model_and_the_oracle(fmt):
    """recording (a): the 100-PRB cell at -9.9 MHz (61.44 -> 30.72 MS/s) and the 25-PRB cell at +17 MHz (61.44 -> 7.68 MS/s, ratio 8), equal amplitude: each cell
    through the float64 model and the CPU oracle returns every record of the oracle's run on that cell's original capture, no code block decided at the last
    turbo iteration.  What licenses the GPU replays of this recording"""
    from ddc_cases import model_resample, quantise
    from srs_streams import edge_blocks, failed_records
    cells, f = wide_recording()
    _, _, x = quantise(f, fmt)
    for sc, tti0, orecs, opt, f0, native in cells:
        sflen = int(native) // 1000
        plan = WidePlan(WIDE_RATE, native, passband_hz(sc["nof_prb"]), LEAD, 0.0)
        assert plan.max_out(len(f)) // sflen >= WIDE_NSF and len(orecs) >= 10 and failed_records(orecs) == []
        recs, trace = _decode(sc, tti0, opt, model_resample(f0, plan, x, 0, WIDE_NSF * sflen), f.shape[1], sflen)
        assert edge_blocks(trace) == [] and failed_records(recs) == []
        assert recs == orecs, "%d PRB: %d records vs %d" % (sc["nof_prb"], len(recs), len(orecs))


def test_round_trip_with_the_neighbour_20_db_stronger_through_the_channel_filter():
    """recording (c): (a) with the 100-PRB cell 20 dB above the 25-PRB cell; the narrow cell through the float64 chain channel filter -> resampler, the stop band
    from la.cells_stopbands"""
    from chanfilt_model import Design, two_stage
    from srs_streams import edge_blocks, failed_records
    cells, f = wide_recording(20.0)
    stops = la.cells_stopbands([c[4] for c in cells], [c[0]["nof_prb"] for c in cells], WIDE_RATE)
    assert stops[1] == 17e6 + 9.9e6 - passband_hz(100)
    x = f.astype(np.complex64).astype(np.complex128)
    sc, tti0, orecs, opt, f0, native = cells[1]
    sflen = int(native) // 1000
    m = Design(WIDE_RATE, passband_hz(25), stops[1])
    plan = WidePlan(WIDE_RATE, native, passband_hz(25), LEAD, 0.0)
    assert plan.max_out(m.max_out(len(f))) // sflen >= WIDE_NSF
    recs, trace = _decode(sc, tti0, opt, two_stage(m, plan, x, f0, WIDE_NSF * sflen), f.shape[1], sflen)
    assert edge_blocks(trace) == [] and failed_records(recs) == []
    assert recs == orecs, "records differ: %d vs %d" % (len(recs), len(orecs))

"""The antenna map (lsn_antenna_map_t) without a device: the recordings of antmap_cases.py through the float64 model of a mapped cut and
the CPU oracle - what licenses the GPU replays of tests/test_gpu_antmap.py - and the parts of the interface that need no GPU: the struct, the acceptance rule per
output, the refusals of the stand-alone entry (which validates in front of its first device call: asked for no output it never makes one) and the span calls."""
import ctypes as C
import math

import numpy as np
import pytest

import ltesniffer_amd as la
from antmap_cases import (FOUR_NSF, FOUR_OFFSET, FOUR_RATE, NATIVE, SFLEN, UL_RECORDINGS, UL_RECORDS, four_antennas, model_map, oracle_ul, plan_for, ul_recording)
from ddc_cases import quantise
from resample_cases import LEAD
from resample_model import Plan, passband_hz
from srs_streams import edge_blocks, failed_records
from wide_resample_model import WidePlan


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
@pytest.mark.parametrize("name", ["30", "61"])
def test_ul_mode_from_one_antenna_through_the_model_and_the_oracle(name, fmt):
    """downlink at +f and uplink at -f of ONE antenna: output 0 cut at +f, output 1 at -f, both from input antenna 0 with the cell's one plan, through the oracle's
    UL_MODE worker: every record of the stream, byte for byte, none of them decided at the edge"""
    sc, tti0, orecs, otrace, rate_in, fc, f = ul_recording(name)
    nsf = UL_RECORDINGS[name][0]
    assert len(orecs) == UL_RECORDS[name] and edge_blocks(otrace) == [] and failed_records(orecs) == []
    assert sum(1 for r in orecs if r[1] == 0) >= 1, "no uplink record"    # (byte 1 of a record's context: the direction, 0 = uplink)
    plan = plan_for(rate_in)
    assert type(plan) is (Plan if name == "30" else WidePlan) and plan.taps == (50 if name == "30" else 100)
    assert plan.max_out(len(f)) // SFLEN >= nsf
    _, _, x = quantise(f, fmt)
    y = model_map(x, rate_in, fc, (0, 0), (0.0, -2.0 * fc), nsf * SFLEN, plan)
    recs, trace = oracle_ul(sc, tti0, y, nsf)
    assert edge_blocks(trace) == [] and failed_records(recs) == []
    assert recs == orecs, "%s MS/s fmt %d: %d records vs %d" % (name, fmt, len(recs), len(orecs))


def test_two_of_four_antennas_through_the_model_and_the_oracle():
    from lsn_testlib import oracle_trace
    from parity import oracle_records, run_oracle
    sc, tti0, orecs, otrace, opt, f = four_antennas()
    assert edge_blocks(otrace) == [] and failed_records(orecs) == [] and len(orecs) >= 10
    x = f.astype(np.complex64).astype(np.complex128)
    plan = plan_for(FOUR_RATE)
    y = model_map(x, FOUR_RATE, FOUR_OFFSET, (2, 3), (0.0, 0.0), FOUR_NSF * SFLEN, plan)
    iq = np.ascontiguousarray(y.reshape(2, FOUR_NSF, SFLEN).transpose(1, 0, 2)).astype(np.complex64)
    _, _, recs = run_oracle(sc, tti0, iq, taps=False, trace=True, **opt)
    recs = oracle_records(recs)
    assert edge_blocks(oracle_trace()) == [] and failed_records(recs) == []
    assert recs == orecs, (len(recs), len(orecs))


# ---- the interface, without a device ----
def test_struct_size():
    assert C.sizeof(la.AntennaMap) == 32 and la.MAP_MAX_OUT == 2
    m = la.antenna_map((1, 0), (0.0, -30e6))
    assert (m.struct_size, m.nof_out, list(m.src_antenna), list(m.offset_hz)) == (32, 2, [1, 0], [0.0, -30e6])
    assert la.antenna_map().nof_out == 0


RATE_IN, B = 30.72e6, passband_hz(25)
X = np.zeros((8, 2), dtype=np.complex64)


def _accepted(center, src, offs, x=X, **kw):
    """the stand-alone entry asked for no output: validated, nothing launched"""
    try:
        out = la.resample_cells_map(x, RATE_IN, [dict(rate_out=NATIVE, passband_hz=B, center_offset_hz=center, src=src, offset_hz=offs, n_out=0, **kw)])
    except ValueError:
        return False
    assert out[0].shape == (len(src), 0)
    return True


def test_acceptance_rule_per_output_at_the_exact_edge():
    edge = RATE_IN / 2 - B        # |center + offset| + B <= rate_in / 2
    above = math.nextafter(edge, math.inf)
    assert _accepted(0.0, (0, 0), (edge, -edge)) and _accepted(0.0, (0,), (edge,)) and _accepted(0.0, (0,), (-edge,))
    assert not _accepted(0.0, (0, 0), (above, 0.0)) and not _accepted(0.0, (0, 0), (0.0, -above)) and not _accepted(0.0, (0,), (above,))
    # the rule is on the SUM: a centre offset outside the recording is brought back by the output's offset, and an inside one carried out
    assert _accepted(edge + 1e6, (0, 0), (-1e6, -2 * edge - 1e6)) and not _accepted(edge, (0, 0), (0.0, 1.0))
    assert _accepted(7.5e6, (0, 0), (0.0, -15e6))
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert not _accepted(0.0, (0, 0), (0.0, bad)) and not _accepted(0.0, (0, 0), (bad, 0.0)) and not _accepted(bad, (0, 0), (0.0, 0.0))


def test_sources_and_output_counts():
    assert _accepted(0.0, (1, 1), (0.0, 0.0)) and _accepted(0.0, (1, 0), (0.0, 0.0)) and _accepted(0.0, (0,), (0.0,))
    assert not _accepted(0.0, (2, 0), (0.0, 0.0)) and not _accepted(0.0, (0, 2), (0.0, 0.0)) and not _accepted(0.0, (0, 0xFFFFFFFF), (0.0, 0.0))
    assert not _accepted(0.0, (0, 0, 0), (0.0, 0.0, 0.0))          # nof_out = 3
    one = np.zeros((8, 1), dtype=np.complex64)
    assert _accepted(0.0, (0, 0), (0.0, 0.0), x=one) and not _accepted(0.0, (0, 1), (0.0, 0.0), x=one)
    # nof_out = 0 is the identity: the cell as lsn_resample_cells takes it, its own acceptance rule included
    ident = dict(rate_out=NATIVE, passband_hz=B, n_out=0)
    assert la.resample_cells_map(X, RATE_IN, [ident])[0].shape == (2, 0)
    with pytest.raises(ValueError):
        la.resample_cells_map(X, RATE_IN, [dict(ident, center_offset_hz=RATE_IN / 2)])
    # a struct_size the library does not know
    L = la.lib()
    cfg = la._resample_cfg(2, RATE_IN, NATIVE, 0, 0.0, 0, 0, B, la.FILE_CF32, 0.0)
    counts, ptrs = (C.c_uint64 * 1)(0), (C.c_void_p * 1)(None)
    for size, want in ((32, 0), (24, -2), (40, -2), (0, -2)):
        m = la.antenna_map((0, 1))
        m.struct_size = size
        assert L.lsn_resample_cells_map(0, X.ctypes.data, 0, 8, C.byref(cfg), C.byref(m), 1, ptrs, 0, counts) == want, size
    assert L.lsn_resample_cells_map(0, X.ctypes.data, 0, 8, C.byref(cfg), None, 1, ptrs, 0, counts) == -2
    with pytest.raises(ValueError):     # the ring's own rule stays
        la.resample_cells_ring_map(X, RATE_IN, [dict(ident, src=(0, 0))], 6)


def _fit(plan, blk, cap):
    """lsn_cells.h: the largest b <= blk whose block-0 span, plus two samples, fits cap"""
    fits = [b for b in range(1, blk + 1) if plan.span(0, b * SFLEN)[1] - plan.span(0, b * SFLEN)[0] + 2 <= cap]
    return fits[-1] if fits else 0


@pytest.mark.parametrize("fmt,bytes_", [(la.FILE_CF32, 8), (la.FILE_SC16, 4)])
@pytest.mark.parametrize("rate_in", [15.36e6, 30.72e6, 61.44e6])
def test_file_span_follows_the_recordings_antennas(rate_in, fmt, bytes_):
    """the raw block buffer is the Phy's - blk_subframes subframes of nof_out antennas of cf32 - and holds ALL antennas of the recording: blk_used follows the
    recording's antenna count, a block's span does not"""
    cell = dict(nof_prb=25, center_offset_hz=1e6, offset_time=LEAD)
    plan = plan_for(rate_in)
    in_end, blk = int(rate_in) // 1000 * 64 + LEAD + 1000, 20
    used = {}
    for nin in (1, 2, 4):
        for rows in (1, 2):
            want = used[nin, rows] = _fit(plan, blk, blk * SFLEN * rows * 8 // (bytes_ * nin))
            if not want:      # not one subframe's input of all the recording's antennas fits the Phy's buffer: refused, as cells too far apart are
                with pytest.raises(ValueError):
                    la.file_cells_span(rate_in, [cell], in_end, blk_subframes=blk, nof_antennas=nin, sample_format=fmt, nof_out=[rows])
                continue
            b0 = la.file_cells_span(rate_in, [cell], in_end, blk_subframes=blk, nof_antennas=nin, sample_format=fmt, nof_out=[rows])
            assert b0["blk_used"] == want, (nin, rows, b0["blk_used"], want)
            done = 0
            for k in range(200):
                b = la.file_cells_span(rate_in, [cell], in_end, block=k, blk_subframes=blk, nof_antennas=nin, sample_format=fmt, nof_out=[rows])
                if not b["nof_active"]:
                    break
                lo, hi = plan.span(done * SFLEN, b["nof_subframes"][0] * SFLEN)
                assert b["first_subframe"] == [done] and (b["in_lo"], b["in_hi"]) == (max(lo, 0), hi) and b["taps"] == [plan.taps]
                done += b["nof_subframes"][0]
            assert done == 64
        # nof_out 0 is the unmapped call: the Phy has the recording's antennas
        old = la.file_cells_span(rate_in, [cell], in_end, blk_subframes=blk, nof_antennas=nin, sample_format=fmt)
        assert old == la.file_cells_span(rate_in, [cell], in_end, blk_subframes=blk, nof_antennas=nin, sample_format=fmt, nof_out=[0])
        if nin <= 2:
            assert old == la.file_cells_span(rate_in, [cell], in_end, blk_subframes=blk, nof_antennas=nin, sample_format=fmt, nof_out=[nin])
    assert used[1, 2] >= used[2, 2] >= used[4, 2] and used[1, 2] > used[4, 2] and used[1, 1] == used[2, 2]
    # two cells, the second unmapped: the largest Phy's buffer is the block's
    two = la.file_cells_span(rate_in, [cell, dict(cell, center_offset_hz=-1e6)], in_end, blk_subframes=blk, nof_antennas=1, sample_format=fmt, nof_out=[2, 0])
    assert two["blk_used"] == used[1, 2]
    for bad in ([3], [0xFFFFFFFF]):
        with pytest.raises(ValueError):
            la.file_cells_span(rate_in, [cell], in_end, blk_subframes=blk, nof_antennas=1, sample_format=fmt, nof_out=bad)
    with pytest.raises(ValueError):
        la.file_cells_span(rate_in, [cell], in_end, blk_subframes=blk, nof_antennas=9, sample_format=fmt, nof_out=[2])


def test_stream_span_does_not_depend_on_either_antenna_count():
    cell = dict(nof_prb=25, center_offset_hz=15e6, offset_time=LEAD)
    ref = la.stream_span(61.44e6, [cell], 61440 * 20, nof_antennas=2, block_subframes=4)
    for nin in (1, 2, 4):
        for rows in (0, 1, 2):
            assert la.stream_span(61.44e6, [cell], 61440 * 20, nof_antennas=nin, block_subframes=4, nof_out=[rows]) == ref
    with pytest.raises(ValueError):
        la.stream_span(61.44e6, [cell], 61440 * 20, nof_antennas=1, block_subframes=4, nof_out=[3])
    with pytest.raises(ValueError):
        la.stream_span(61.44e6, [cell], 61440 * 20, nof_antennas=1, block_subframes=4, nof_out=[2], stopbands=[3e6])

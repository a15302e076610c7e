"""The plan of a multi-cell file replay (lsn_file_cells_span: host/lsn_cells.cc), without a GPU: block k of the replay is the same output subframes of
every cell, fed from the UNION of the cells' input spans; the block size shrinks until the union fits the raw block buffer; a cell that has run out drops out;
what cannot be replayed in one pass is refused.  And the round trip of a recording that holds a 75-PRB and a 25-PRB cell through the float64 model and the CPU
oracle - what licenses the GPU replay of that recording (test_gpu_cells.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import ltesniffer_amd as la
from resample_model import passband_hz

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
SF = {100: 30720, 75: 23040, 50: 15360, 25: 7680}   # output samples of one subframe (3GPP rates)


def _single(rate_in, c, sf0, nsf, in_end):
    """la.resample_span of the output subframes [sf0, sf0 + nsf) of one cell, and how many whole subframes lie inside the recording"""
    n = SF[c["nof_prb"]]
    kw = dict(first_sample=c.get("offset_time", 0) + int(c.get("offset_time_frac", 0.0)), first_frac=c.get("offset_time_frac", 0.0) % 1.0, passband_hz=passband_hz(c["nof_prb"]),
              center_offset_hz=c.get("center_offset_hz", 0.0))
    sp = la.resample_span(nsf * n, in_end, rate_in, 1000.0 * n, out_first=sf0 * n, **kw)
    whole = la.resample_span(0, in_end, rate_in, 1000.0 * n, **kw)["max_out"] // n
    return sp, whole


def _blocks(rate_in, cells, in_end, blk, **kw):
    out = []
    for k in range(10 ** 6):
        b = la.file_cells_span(rate_in, cells, in_end, block=k, blk_subframes=blk, **kw)
        if not b["nof_active"]:
            assert b["in_lo"] == b["in_hi"] == 0 and not any(b["nof_subframes"])
            return out
        out.append(b)
    raise AssertionError("the replay does not end")


def _check_union(rate_in, cells, in_end, blocks):
    """every block: per cell the subframes and taps of its single-cell plan, and the union = min / max of the single spans of the cells that take part"""
    for k, b in enumerate(blocks):
        los, his = [], []
        for c, sf0, nsf, taps in zip(cells, b["first_subframe"], b["nof_subframes"], b["taps"]):
            if not nsf:
                continue
            sp, whole = _single(rate_in, c, sf0, nsf, in_end)
            total = min(whole, c.get("max_subframes") or whole)
            assert sf0 == k * b["blk_used"] and nsf == min(b["blk_used"], total - sf0) and taps == sp["taps"], (k, c)
            los.append(sp["in_lo"])
            his.append(sp["in_hi"])
        assert b["nof_active"] == len(los) > 0
        assert (b["in_lo"], b["in_hi"]) == (max(min(los), 0), max(his)), k
        assert b["in_hi"] <= in_end


def _check_fit(rate_in, cells, in_end, blk, used, cap):
    """blk shrank to `used`: the union of block 0 with `used` subframes of every cell fits the buffer of cap samples with the two samples of slack the plan keeps
    for later blocks, and - unless nothing had to shrink - one subframe more would not"""
    def union(n):
        sp = [_single(rate_in, c, 0, n, 10 ** 12)[0] for c in cells]
        return max(s["in_hi"] for s in sp) - min(s["in_lo"] for s in sp)
    assert 1 <= used <= blk and union(used) + 2 <= cap and (used == blk or union(used + 1) + 2 > cap), (used, blk, cap)


def test_the_mirror_is_the_header_struct():
    assert C.sizeof(la.FileCell) == 88 and C.sizeof(la.FileCellsSpan) == 8 + 8 + 8 + 8 * 8 + 8 * 4 + 8 * 4 and la.FILE_MAX_CELLS == 8


@pytest.mark.parametrize("fmt", [la.FILE_CF32, la.FILE_SC16])
def test_one_cell_is_the_single_cell_plan(fmt):
    rate_in, in_end = 25e6, 25000 * 23 + 500
    c = dict(nof_prb=100, center_offset_hz=1.5e6, offset_time=1000, offset_time_frac=0.375)
    blocks = _blocks(rate_in, [c], in_end, 5, sample_format=fmt)
    _check_union(rate_in, [c], in_end, blocks)
    assert sum(b["nof_subframes"][0] for b in blocks) == _single(rate_in, c, 0, 1, in_end)[1] == 22
    assert all(b["blk_used"] == 5 for b in blocks)     # 25 -> 30.72 MS/s: the input of a block is smaller than its output


@pytest.mark.parametrize("dt,frac", [(0, 0.0), (7, 0.25), (3 * 61440, 0.0)])
def test_two_cells_of_equal_bandwidth_share_the_union_of_their_spans(dt, frac):
    rate_in, in_end, blk = 61.44e6, 61440 * 40 + 2000, 16
    cells = [dict(nof_prb=100, center_offset_hz=9.9e6, offset_time=1000), dict(nof_prb=100, center_offset_hz=-9.9e6, offset_time=1000 + dt, offset_time_frac=frac)]
    blocks = _blocks(rate_in, cells, in_end, blk, sample_format=la.FILE_SC16)
    _check_union(rate_in, cells, in_end, blocks)
    assert len(blocks) >= 3 and [sum(b["nof_subframes"][i] for b in blocks) for i in (0, 1)] == [40, 40 - (3 if dt > 7 else 0)]
    # sc16: the buffer of 16 subframes of cf32 output holds 16 subframes' worth of 61.44 MS/s input samples, less the filter's length: 15, and 12 when the
    # cells start 3 subframes apart
    used = blocks[0]["blk_used"]
    _check_fit(rate_in, cells, in_end, blk, used, blk * 30720 * 2)
    assert used == (15 if dt <= 7 else 12) and all(b["blk_used"] == used and b["in_hi"] - b["in_lo"] <= blk * 30720 * 2 for b in blocks)
    T = max(blocks[0]["taps"])
    for a, b in zip(blocks, blocks[1:]):
        if b["nof_active"] == 2:
            assert 0 < a["in_hi"] - b["in_lo"] <= T + math.ceil(dt + frac), (a, b)     # consecutive unions overlap by no more than the larger T plus the start difference


def test_mixed_bandwidths_keep_the_single_cell_plans_and_shrink_the_block():
    rate_in, in_end = 30.72e6, 30720 * 20 + 2000
    cells = [dict(nof_prb=75, center_offset_hz=-4.5e6, offset_time=1000), dict(nof_prb=25, center_offset_hz=7.5e6, offset_time=1000, max_subframes=20)]
    for fmt, blk, used in ((la.FILE_CF32, 8, 5), (la.FILE_SC16, 8, 8), (la.FILE_CF32, 1, None)):     # 8 x 23 040 samples hold 5 subframes of 30 720 and the filter
        if used is None:     # one subframe of 30.72 MS/s cf32 input does not fit a buffer of one 23.04 MS/s subframe: refused, as the single-cell call refuses it
            with pytest.raises(ValueError):
                la.file_cells_span(rate_in, cells, in_end, 0, blk, sample_format=fmt)
            continue
        blocks = _blocks(rate_in, cells, in_end, blk, sample_format=fmt)
        _check_union(rate_in, cells, in_end, blocks)
        assert blocks[0]["taps"] == [_single(rate_in, c, 0, 1, in_end)[0]["taps"] for c in cells] and blocks[0]["taps"][0] != blocks[0]["taps"][1]
        assert [sum(b["nof_subframes"][i] for b in blocks) for i in (0, 1)] == [20, 20]
        # the raw buffer holds blk subframes of cf32 of the WIDEST cell (23 040 samples): no union is longer than that, and blk shrank to make it so
        cap = blk * 23040 * 8 // (8, 4)[fmt]
        assert all(b["blk_used"] == used and b["in_hi"] - b["in_lo"] <= cap for b in blocks)
        _check_fit(rate_in, cells, in_end, blk, used, cap)


def test_a_cell_with_fewer_subframes_drops_out_and_the_union_narrows():
    rate_in, in_end = 61.44e6, 61440 * 24 + 2000
    cells = [dict(nof_prb=100, center_offset_hz=9.9e6, offset_time=1000, max_subframes=7), dict(nof_prb=100, center_offset_hz=-9.9e6, offset_time=1000 + 3 * 61440)]
    blocks = _blocks(rate_in, cells, in_end, 10, sample_format=la.FILE_SC16)
    _check_union(rate_in, cells, in_end, blocks)
    used = blocks[0]["blk_used"]
    assert [sum(b["nof_subframes"][i] for b in blocks) for i in (0, 1)] == [7, 21] and used < 7
    assert [b["nof_active"] for b in blocks] == [2, 2] + [1] * (len(blocks) - 2)
    last = blocks[2]
    sp, _ = _single(rate_in, cells[1], last["first_subframe"][1], last["nof_subframes"][1], in_end)
    assert (last["in_lo"], last["in_hi"]) == (sp["in_lo"], sp["in_hi"]) and last["nof_subframes"][0] == 0


def _rc(cells, n=None, rate=61.44e6, fc=None, in_end=61440 * 12, blk=5, out=True):
    arr = (la.FileCell * 16)()
    for i, c in enumerate(cells or []):
        arr[i] = c
    fc = fc or la.FileCfg(2, 0, 0.0, la.FILE_CF32, 0.0)
    sp = la.FileCellsSpan()
    return la.lib().lsn_file_cells_span(C.byref(fc) if fc != "null" else None, rate, arr if cells is not None else None, len(cells or []) if n is None else n, in_end, 0, blk,
                                        C.byref(sp) if out else None)


def test_every_refusal_that_needs_no_device():
    def cell(**kw):
        return la._file_cell(None, dict(dict(nof_prb=100, center_offset_hz=9.9e6, offset_time=1000), **kw))
    a, b = cell(), cell(center_offset_hz=-9.9e6)
    assert _rc([a, b]) == 0 and _rc([a] * 8) == 0
    assert _rc([a] * 9) == INVALID and _rc([a, b], n=0) == INVALID                              # n_cells 0 or above LSN_FILE_MAX_CELLS
    for size in (84, 92, 0):                                                                     # a struct_size off by 4
        bad = cell()
        bad.struct_size = size
        assert _rc([a, bad]) == INVALID, size
    assert _rc([a, cell(offset_time=1000 + 10000 * 61440)], in_end=61440 * 20000) == INVALID     # starts 10 000 subframes apart: no block holds one subframe of each
    assert _rc([a, cell(offset_time=1000 + 61440)], blk=5) == 0 and _rc([a, cell(offset_time=1000 + 2 * 61440)], blk=5) == INVALID   # (2 x 5 / 2 subframes of input fit)
    for fc in (la.FileCfg(2, 1, 0.0, 0, 0.0), la.FileCfg(2, 0, 100.0, 0, 0.0), la.FileCfg(2, 0, 0.0, 3, 0.0), la.FileCfg(0, 0, 0.0, 0, 0.0), la.FileCfg(2, 0, 0.0, 1, -1.0), "null"):
        assert _rc([a, b], fc=fc) == INVALID                                                      # the offset fields of cfg must be 0; format and antennas as ever
    # a cell the single-cell call would refuse: outside the recording, a negative or non-finite start, a rate the filter does not meet, no such bandwidth
    edge = 61.44e6 / 2 - passband_hz(100)
    for bad in (cell(center_offset_hz=edge + 1.0), cell(center_offset_hz=float("nan")), cell(offset_time=-1), cell(offset_time_frac=-0.5), cell(offset_time_frac=float("inf")),
                cell(nof_prb=99), cell(rates=7), cell(offset_freq=float("nan"))):
        assert _rc([a, bad]) == INVALID and _rc([bad]) == INVALID
    assert _rc([a, b], rate=130e6) == INVALID and _rc([a, b], rate=0.0) == INVALID and _rc([a, b], rate=float("nan")) == INVALID
    assert _rc([a, b], blk=0) == INVALID and _rc([a, b], out=False) == INVALID and _rc(None, n=2) == INVALID
    with pytest.raises(ValueError):
        la.file_cells_span(61.44e6, [dict(nof_prb=100), dict(nof_prb=100, offset_time=10000 * 61440)], 61440 * 20000)
    with pytest.raises(ValueError):     # process_file_cells refuses in front of the library's first device call: no Phy
        la.process_file_cells("/nonexistent", 61.44e6, [], nof_antennas=2)


def test_round_trip_of_the_mixed_recording_through_the_model_and_the_oracle():
    """a 75-PRB cell at -4.5 MHz and a 25-PRB cell at +7.5 MHz of one 30.72 MS/s recording, equal amplitude: each cell through the float64 model (mixer + its
    own filter, 30.72 -> 23.04 and 30.72 -> 7.68 MS/s) and the CPU oracle returns every record of the oracle's run on that cell's original capture"""
    from cells_cases import MIXED_NSF, MIXED_RATE, mixed_recording
    from ddc_cases import model_resample
    from parity import oracle_records, run_oracle
    from resample_cases import LEAD
    from resample_model import Plan
    from srs_streams import failed_records
    cells, f = mixed_recording()
    x = f.astype(np.complex64).astype(np.complex128)
    # where the replay puts the cells: both start at sample LEAD, the 25-PRB cell is cut by max_subframes; the plan says how many subframes of each lie in the file
    placed = [dict(nof_prb=sc["nof_prb"], center_offset_hz=f0, offset_time=LEAD, max_subframes=MIXED_NSF if sc["nof_prb"] == 25 else 0) for sc, _, _, _, f0, _ in cells]
    blocks = _blocks(MIXED_RATE, placed, len(f), 8, nof_antennas=f.shape[1])
    assert [sum(b["nof_subframes"][i] for b in blocks) for i in (0, 1)] == [MIXED_NSF, MIXED_NSF] and blocks[-1]["in_hi"] <= len(f)
    for sc, tti0, orecs, opt, f0, native in cells:
        sflen = int(native) // 1000
        plan = Plan(MIXED_RATE, native, passband_hz(sc["nof_prb"]), LEAD, 0.0)
        assert plan.max_out(len(f)) // sflen >= MIXED_NSF
        y = model_resample(f0, plan, x, 0, MIXED_NSF * sflen)
        iq = np.ascontiguousarray(y.reshape(MIXED_NSF, sflen, f.shape[1]).transpose(0, 2, 1)).astype(np.complex64)
        _, _, recs = run_oracle(sc, tti0, iq, taps=False, **opt)
        recs = oracle_records(recs)
        assert len(orecs) >= 10 and failed_records(orecs) == []
        assert recs == orecs, "%d PRB: %d records vs %d" % (sc["nof_prb"], len(recs), len(orecs))

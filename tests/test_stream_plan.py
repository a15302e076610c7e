"""The plan of a pushed stream (lsn_stream_span: host/lsn_stream.cc), without a GPU: after `pushed` samples a cell has the complete subframes a file
of that length replays; a stream that is never flushed submits them in whole blocks; the oldest sample any cell still needs is the first input sample of the next
unsubmitted subframe of the cell that is furthest behind, and a cell that has run out no longer holds it back; the ring is a power of two that holds a block of
every cell; and what cannot be streamed is refused.  Every comparison is an equality of integers."""
import ctypes as C

import pytest

import ltesniffer_amd as la
from resample_model import passband_hz

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
SF = {100: 30720, 75: 23040, 50: 15360, 25: 7680}   # output samples of one subframe (3GPP rates)
LEAD = 1000
# the two-cell 61.44 MS/s recording (ddc_cases "two_cells_*": LEAD + 12 subframes + 1000 samples) and the mixed 75 / 25-PRB one (cells_cases: 30.72 MS/s, the
# 25-PRB cell cut to 20 subframes), as the file tests place their cells
TWO = (61.44e6, LEAD + 12 * 61440 + 1000, [dict(nof_prb=100, center_offset_hz=9.9e6, offset_time=LEAD), dict(nof_prb=100, center_offset_hz=-9.9e6, offset_time=LEAD)])
MIXED = (30.72e6, LEAD + 20 * 30720 + 1000, [dict(nof_prb=75, center_offset_hz=-4.5e6, offset_time=LEAD), dict(nof_prb=25, center_offset_hz=7.5e6, offset_time=LEAD, max_subframes=20)])


def _lo(rate_in, c, sf):
    """first input sample subframe sf of the cell reads, clamped at the start of the stream"""
    n = SF[c["nof_prb"]]
    sp = la.resample_span(n, 10 ** 12, rate_in, 1000.0 * n, first_sample=c.get("offset_time", 0), out_first=sf * n, passband_hz=passband_hz(c["nof_prb"]),
                          center_offset_hz=c.get("center_offset_hz", 0.0))
    return max(sp["in_lo"], 0)


def _union(rate_in, cells, blk):
    sp = []
    for c in cells:
        n = SF[c["nof_prb"]]
        sp.append(la.resample_span(blk * n, 10 ** 12, rate_in, 1000.0 * n, first_sample=c.get("offset_time", 0), passband_hz=passband_hz(c["nof_prb"]),
                                   center_offset_hz=c.get("center_offset_hz", 0.0)))
    return max(s["in_hi"] for s in sp) - min(s["in_lo"] for s in sp)


def _file_totals(rate_in, cells, in_end):
    """subframes per cell that process_file_cells replays of a file of in_end samples: file_cells_span summed over its blocks"""
    tot = [0] * len(cells)
    for k in range(10 ** 6):
        b = la.file_cells_span(rate_in, cells, in_end, block=k, blk_subframes=64)
        if not b["nof_active"]:
            return tot
        tot = [t + n for t, n in zip(tot, b["nof_subframes"])]
    raise AssertionError("the replay does not end")


def test_the_mirrors_are_the_header_structs_and_the_symbols_exist():
    assert C.sizeof(la.StreamCfg) == 40 and C.sizeof(la.StreamStatus) == 136 and C.sizeof(la.StreamSpan) == 200
    for s in ("lsn_stream_open", "lsn_stream_push", "lsn_stream_flush", "lsn_stream_status", "lsn_stream_close", "lsn_stream_span", "lsn_resample_cells_ring"):
        assert s in la.EXPORTS
        getattr(la.lib(), s)


@pytest.mark.parametrize("case", [TWO, MIXED], ids=["two_cells", "mixed"])
@pytest.mark.parametrize("blk", [1, 5])
def test_subframes_grow_with_the_samples_and_end_at_the_file_replays_totals(case, blk):
    rate_in, in_end, cells = case
    prev = None
    grid = sorted(set(list(range(0, in_end, 4099)) + [in_end - 1, in_end]))
    for pushed in grid:
        s = la.stream_span(rate_in, cells, pushed, block_subframes=blk)
        comp, sub = s["subframes_complete"], s["subframes_submitted"]
        if prev is not None:
            assert all(a <= b for a, b in zip(prev[0], comp)) and all(a <= b for a, b in zip(prev[1], sub)), pushed     # non-decreasing in pushed
        for c, k, d in zip(cells, comp, sub):
            # never flushed: whole blocks, and the last subframes in front of max_subframes
            assert d == (k if c.get("max_subframes") and k == c["max_subframes"] else k // blk * blk), (pushed, k, d)
        # the oldest sample a cell still needs: the first input sample of the next unsubmitted subframe, minimised over the cells that have not run out
        live = [_lo(rate_in, c, d) for c, d in zip(cells, sub) if not (c.get("max_subframes") and d >= c["max_subframes"])]
        assert s["oldest_needed"] == (min(min(live), pushed) if live else pushed), pushed
        assert all(s["oldest_needed"] <= lo for lo in live)
        live = [_lo(rate_in, c, k) for c, k in zip(cells, comp) if not (c.get("max_subframes") and k >= c["max_subframes"])]
        assert s["oldest_needed_flushed"] == (min(min(live), pushed) if live else pushed) and s["oldest_needed"] <= s["oldest_needed_flushed"]
        prev = (comp, sub)
    # a stream that received in_end samples in all has, per cell, the subframes a file of in_end samples replays
    want = _file_totals(rate_in, cells, in_end)
    assert prev[0] == want and min(want) >= 12, (prev, want)


def test_a_cell_that_has_run_out_no_longer_holds_the_oldest_sample_back():
    rate_in, in_end = 61.44e6, LEAD + 24 * 61440 + 1000
    a = dict(nof_prb=100, center_offset_hz=9.9e6, offset_time=LEAD, max_subframes=7)
    b = dict(nof_prb=100, center_offset_hz=-9.9e6, offset_time=LEAD + 3 * 61440 + 5000)
    stuck = _lo(rate_in, a, 7)     # what a plan that went on counting cell a would report at the end
    seen = set()
    for pushed in range(0, in_end + 1, 20011):
        s = la.stream_span(rate_in, [a, b], pushed, block_subframes=1)
        da, db = s["subframes_submitted"]
        seen.add(da)
        if da < 7:
            assert s["oldest_needed"] == min(_lo(rate_in, a, da), _lo(rate_in, b, db), pushed)
        else:
            assert da == 7 and s["oldest_needed"] == min(_lo(rate_in, b, db), pushed)
    assert seen == set(range(8))
    end = la.stream_span(rate_in, [a, b], in_end, block_subframes=1)
    assert end["subframes_submitted"] == [7, 20] and end["oldest_needed"] == _lo(rate_in, b, 20) > stuck
    # every cell has run out: nothing is needed any more
    b["max_subframes"] = 20
    assert la.stream_span(rate_in, [a, b], in_end, block_subframes=1)["oldest_needed"] == in_end


@pytest.mark.parametrize("blk", [1, 5, 16])
def test_the_default_ring_is_the_smallest_power_of_two_that_holds_four_blocks_of_the_union(blk):
    for rate_in, _, cells in (TWO, MIXED):
        s = la.stream_span(rate_in, cells, 0, block_subframes=blk)
        assert s["block_subframes"] == blk and s["block_input"] == _union(rate_in, cells, blk) + 2
        ring = s["ring_samples"]
        assert ring & (ring - 1) == 0 and ring >= 4 * s["block_input"] > ring // 2
        assert s["taps"] == [la.resample_span(0, 10 ** 9, rate_in, 1000.0 * SF[c["nof_prb"]], passband_hz=passband_hz(c["nof_prb"]))["taps"] for c in cells]
        # the smallest ring the library accepts holds one block
        small = 1 << (s["block_input"] - 1).bit_length()
        assert la.stream_span(rate_in, cells, 0, block_subframes=blk, ring_samples=small)["ring_samples"] == small
        with pytest.raises(ValueError):
            la.stream_span(rate_in, cells, 0, block_subframes=blk, ring_samples=small // 2)


def _rc(cells, n=None, rate=61.44e6, blk=1, ring=0, size=None, nant=2, fmt=la.FILE_CF32, pushed=0, out=True, cfg=True):
    arr = (la.FileCell * 16)()
    for i, c in enumerate(cells or []):
        arr[i] = c
    sc = la.StreamCfg(C.sizeof(la.StreamCfg) if size is None else size, 0, rate, nant, fmt, 0.0, blk, ring)
    sp = la.StreamSpan()
    return la.lib().lsn_stream_span(C.byref(sc) if cfg else None, arr if cells is not None else None, len(cells or []) if n is None else n, pushed, C.byref(sp) if out else None)


def test_every_refusal_that_needs_no_device(monkeypatch):
    monkeypatch.delenv("LSN_FILE_BLOCK", raising=False)     # the file source's block size is its default, 800
    def cell(**kw):
        return la._file_cell(None, dict(dict(nof_prb=100, center_offset_hz=9.9e6, offset_time=LEAD), **kw))
    a, b = cell(), cell(center_offset_hz=-9.9e6)
    assert _rc([a, b]) == 0 and _rc([a] * 8) == 0
    assert _rc([a, b], ring=100000) == INVALID and _rc([a, b], ring=3 << 16) == INVALID      # a ring size that is not a power of two
    assert _rc([a, b], ring=1 << 16) == 0 and _rc([a, b], ring=1 << 15) == INVALID           # one subframe of 61 440 input samples and the filter: 65 536 hold it, 32 768 do not
    assert _rc([a, b], blk=5, ring=1 << 18) == INVALID and _rc([a, b], blk=5, ring=1 << 19) == 0   # a ring smaller than one block of every cell
    assert _rc([a, b], ring=1 << 33) == INVALID                                              # the ring mask is 32 bits wide
    # starts too far apart: the ring must hold a block of every cell between the oldest start and the newest data
    far = 1 << 20
    assert _rc([a, cell(offset_time=LEAD + far - 61440 - 200)], ring=far) == 0 and _rc([a, cell(offset_time=LEAD + far - 61440 + 200)], ring=far) == INVALID
    assert _rc([a, cell(offset_time=LEAD + 10000 * 61440)]) == 0 and _rc([a, cell(offset_time=LEAD + (1 << 31))]) == INVALID   # (default ring: four blocks, at most 2^32)
    assert _rc([a, cell(start_tti=la.TTI_FROM_MIB)]) == INVALID and _rc([cell(start_tti=la.TTI_FROM_MIB)]) == INVALID
    assert _rc([a] * 9) == INVALID and _rc([a, b], n=0) == INVALID and _rc(None, n=2) == INVALID
    assert _rc([a, b], blk=800) == 0 and _rc([a, b], blk=801) == INVALID                     # block_subframes above the file source's block size
    assert _rc([a, b], size=36) == INVALID and _rc([a, b], size=44) == INVALID and _rc([a, b], cfg=False) == INVALID and _rc([a, b], out=False) == INVALID
    # everything the file pass refuses: format and antennas, the rate, a cell its single-cell call refuses, a struct_size off by 4
    assert _rc([a, b], fmt=3) == INVALID and _rc([a, b], nant=0) == INVALID and _rc([a, b], rate=130e6) == INVALID and _rc([a, b], rate=float("nan")) == INVALID
    for bad in (cell(center_offset_hz=25e6), cell(offset_time=-1), cell(offset_time_frac=float("inf")), cell(nof_prb=99), cell(offset_freq=float("nan"))):
        assert _rc([a, bad]) == INVALID
    bad = cell()
    bad.struct_size = 84
    assert _rc([a, bad]) == INVALID
    with pytest.raises(ValueError):
        la.stream_span(61.44e6, [dict(nof_prb=100), dict(nof_prb=100)], 0, ring_samples=12345)
    with pytest.raises(ValueError):     # Stream refuses in front of the library's first device call: no Phy
        la.Stream(61.44e6, [], nof_antennas=2)

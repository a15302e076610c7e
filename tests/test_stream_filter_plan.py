"""The plan of a pushed stream with the channel filter on (lsn_stream_span_filtered: host/lsn_stream.cc), without a GPU: every span is the composition
of the two existing span helpers - the resampler's span of a cell's subframes, then the filter's span of exactly those y1 -, a cell's subframes are counted in front
of pushed - L, the ring holds a block of the widened spans, and what cannot be streamed is refused.  Every comparison of the plan is an equality of integers.
Then the float64 chain (stage-1 model -> model detector and loop -> float64 sampler -> CPU oracle) of the two tracked cases test_gpu_stream_filter.py runs: what
the GPU has to decode is established here first."""
import ctypes as C

import pytest

import ltesniffer_amd as la
from chanfilt_cases import B100, RATE, STOP
from resample_model import passband_hz
from stream_filter_cases import LEAD, SF, TWO, chain_drifting, chain_strong_neighbour, complete, half_len, mixed, wide_span

INVALID = -2   # LSN_ERROR_INVALID_INPUTS
CASES = [TWO, mixed()]


def test_the_symbols_exist_and_no_struct_grew():
    assert C.sizeof(la.StreamCfg) == 40 and C.sizeof(la.StreamSpan) == 200 and C.sizeof(la.ChannelFilterCfg) == 64 and C.sizeof(la.FileCell) == 88
    for s in ("lsn_stream_span_filtered", "lsn_channel_filter_ring"):
        assert s in la.EXPORTS
        getattr(la.lib(), s)


def test_the_filters_of_the_two_sets():
    rate, _, cells, stops = TWO
    assert [half_len(rate, c, s) for c, s in zip(cells, stops)] == [88, 88]
    rate, _, cells, stops = CASES[1]
    assert stops == [12e6 - passband_hz(25), 12e6 - passband_hz(75)]             # the distance to the other cell's nearest occupied edge
    assert [half_len(rate, c, s) for c, s in zip(cells, stops)] == [26, 26]      # both transition bands are 2.97 MHz of 30.72 MS/s wide


@pytest.mark.parametrize("case", CASES, ids=["two_cells", "mixed"])
@pytest.mark.parametrize("blk", [1, 5, 16])
def test_counts_and_oldest_needed_are_the_composition_of_the_span_helpers(case, blk):
    rate_in, in_end, cells, stops = case
    prev = None
    for pushed in sorted(set(list(range(0, in_end, 4099)) + [0, 1, 87, 88, 89, in_end - 1, in_end])):
        s = la.stream_span(rate_in, cells, pushed, block_subframes=blk, stopbands=stops)
        comp, sub = s["subframes_complete"], s["subframes_submitted"]
        assert comp == [complete(rate_in, c, S, pushed) for c, S in zip(cells, stops)], pushed
        if prev is not None:
            assert all(a <= b for a, b in zip(prev, comp))
        for c, k, d in zip(cells, comp, sub):     # never flushed: whole blocks, and the last subframes in front of max_subframes
            assert d == (k if c.get("max_subframes") and k == c["max_subframes"] else k // blk * blk), (pushed, k, d)
        for key, counts in (("oldest_needed", sub), ("oldest_needed_flushed", comp)):
            live = [max(wide_span(rate_in, c, S, d, 1)[0], 0) for c, S, d in zip(cells, stops, counts) if not (c.get("max_subframes") and d >= c["max_subframes"])]
            assert s[key] == (min(min(live), pushed) if live else pushed), (key, pushed)
        # a filtered cell is never ahead of the unfiltered one, and at most the subframe that the last L samples complete behind it
        plain = la.stream_span(rate_in, cells, pushed, block_subframes=blk)["subframes_complete"]
        assert all(p - 1 <= k <= p for k, p in zip(comp, plain)), (pushed, comp, plain)
        prev = comp
    assert min(prev) >= 12


@pytest.mark.parametrize("blk", [1, 5, 16])
def test_block_input_and_the_rings_follow_from_the_widened_spans(blk):
    for rate_in, _, cells, stops in CASES:
        s = la.stream_span(rate_in, cells, 0, block_subframes=blk, stopbands=stops)
        spans = [wide_span(rate_in, c, S, 0, blk) for c, S in zip(cells, stops)]
        assert s["block_subframes"] == blk and s["block_input"] == max(h for _, h in spans) - min(l for l, _ in spans) + 2
        plain = la.stream_span(rate_in, cells, 0, block_subframes=blk)
        L = [half_len(rate_in, c, S) for c, S in zip(cells, stops)]
        assert L[0] == L[1] and s["block_input"] == plain["block_input"] + 2 * L[0] and s["taps"] == plain["taps"]
        ring = s["ring_samples"]
        assert ring & (ring - 1) == 0 and ring >= 4 * s["block_input"] > ring // 2           # the smallest power of two that holds four of them
        small = 1 << (s["block_input"] - 1).bit_length()
        assert la.stream_span(rate_in, cells, 0, block_subframes=blk, ring_samples=small, stopbands=stops)["ring_samples"] == small
        with pytest.raises(ValueError):      # one power of two below block_input
            la.stream_span(rate_in, cells, 0, block_subframes=blk, ring_samples=small // 2, stopbands=stops)


def test_a_ring_that_holds_the_plain_block_and_not_the_widened_one_is_refused():
    """the second cell starts so much later that one block of both cells ends 3 samples short of 65 536: it opens without the filter, not with 2 x 88 more"""
    rate_in, _, cells, stops = TWO
    need = la.stream_span(rate_in, cells, 0, block_subframes=1)["block_input"]
    late = [cells[0], dict(cells[1], offset_time=LEAD + 65536 - need - 3)]
    assert la.stream_span(rate_in, late, 0, block_subframes=1, ring_samples=65536)["block_input"] == 65533
    with pytest.raises(ValueError):
        la.stream_span(rate_in, late, 0, block_subframes=1, ring_samples=65536, stopbands=stops)
    assert la.stream_span(rate_in, late, 0, block_subframes=1, ring_samples=131072, stopbands=stops)["block_input"] == 65533 + 176


def test_none_and_zeros_are_todays_answers_and_mixes_and_bad_stop_bands_are_refused():
    rate_in, in_end, cells, stops = TWO
    for pushed in (0, 5000, 70000, in_end):
        for blk in (1, 5):
            plain = la.stream_span(rate_in, cells, pushed, block_subframes=blk)
            assert la.stream_span(rate_in, cells, pushed, block_subframes=blk, stopbands=None) == plain
            assert la.stream_span(rate_in, cells, pushed, block_subframes=blk, stopbands=[0.0, 0.0]) == plain
    for bad in ([STOP, 0.0], [0.0, STOP],                    # a filtered / unfiltered mix
                [STOP, B100], [STOP, B100 - 1.0],            # S <= B
                [STOP, RATE / 2 + 1.0],                      # S > R / 2
                [STOP, B100 + 100e3],                        # L > 512
                [STOP, float("nan")], [STOP, -1.0]):
        with pytest.raises(ValueError):
            la.stream_span(rate_in, cells, 0, stopbands=bad)
    with pytest.raises(ValueError):                          # the cell does not lie inside the band
        la.stream_span(rate_in, [cells[0], dict(cells[1], center_offset_hz=-25e6)], 0, stopbands=[STOP, STOP])
    with pytest.raises(ValueError):                          # TTI_FROM_MIB stays refused
        la.stream_span(rate_in, [cells[0], dict(cells[1], start_tti=la.TTI_FROM_MIB)], 0, stopbands=[STOP, STOP])
    with pytest.raises(ValueError):
        la.stream_span(rate_in, cells, 0, stopbands=[STOP])
    # the C entry: a null list is lsn_stream_span
    arr = (la.FileCell * 2)(*[la._file_cell(None, c) for c in cells])
    cfg = la._stream_cfg(rate_in, 2, la.FILE_CF32, 0.0, 1, 0, 0)
    a, b = la.StreamSpan(), la.StreamSpan()
    assert la.lib().lsn_stream_span_filtered(C.byref(cfg), arr, 2, None, 70000, C.byref(a)) == 0 and la.lib().lsn_stream_span(C.byref(cfg), arr, 2, 70000, C.byref(b)) == 0
    assert bytes(a) == bytes(b)
    assert la.lib().lsn_stream_span_filtered(C.byref(cfg), arr, 2, (C.c_double * 2)(STOP, STOP), 70000, None) == INVALID


# ---- the float64 chain of the tracked cases (run on the GPU by tests/test_gpu_stream_filter.py) ----

def test_chain_a_strong_neighbour_clock_right_loop_on():
    """both cells of the recording whose other carrier is 20 dB stronger through stage-1 model, model loop, float64 sampler and the oracle: every record of the
    oracle's run on each cell's own capture - 69 (B, the weak one) and 66 (A)"""
    for sc, tti0, opt, orecs, recs, log in chain_strong_neighbour():
        print("cell %d: chain %d of %d records; loop log %r" % (sc["cell_id"], len(recs), len(orecs), log))
        assert len(orecs) in (66, 69) and recs == orecs
        assert sum(1 for ok, _, _ in log if ok) >= 2 and all(abs(e) < 8.0 for _, e, _ in log)       # N = 2048: d = 16, the right lag was picked


def test_chain_b_drifting_clock_with_the_filter():
    """the 400-subframe 25-PRB recording made at 10 MS/s by a clock that is off by 60 ppm and slews to 80, with S = 3.5 MHz (L = 21) and initial_ppm = 60: all
    1040 records"""
    assert la.channel_filter_design(10e6, passband_hz(25), 3.5e6)["L"] == 21
    orecs, recs, log = chain_drifting()
    print("drifting recording with the filter: chain %d of %d records; largest |e| %.3f" % (len(recs), len(orecs), max(abs(e) for _, e, _ in log)))
    assert len(orecs) == 1040 and recs == orecs
    assert all(ok for ok, _, _ in log)

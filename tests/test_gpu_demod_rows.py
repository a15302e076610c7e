"""k_pdsch_demod's dense row mapping (16 consecutive (symbol, allocated PRB) rows of one job per workgroup, lsn_rows.h) and its one transmit-diversity element
per lane, against the oracle: every stage-A tap, every stage-C tap (bit-identical int16 soft bits, de-rate-matched words, verdicts) and the record stream, with
the driver of tests/test_gpu_parity.py.  The shapes are the smallest at which the mapping can go wrong; what each capture must contain is asserted on the
transmitter's truth list before anything runs on the GPU (the seeds were picked on that list)."""
import pytest

from lsn_testlib import scenario
from parity import gen_subframes
from test_gpu_parity import _run

pytestmark = pytest.mark.gpu

FMT1, FMT1A, FMT2, FMT2A = 1, 2, 6, 7   # tools/txgen: TXG_FMT*


def _downlink(scn, nsf, seed, **over):
    """-> [(subframe index 0 .. 9, PDU)] of the downlink grants the transmitter sends in this capture"""
    sc = scenario(scn, seed=seed, **over)
    tti0, _, truth = gen_subframes(sc, nsf)
    return [((tti0 + i) % 10, p) for i, pdus in enumerate(truth) for p in pdus if not p["is_ul"]]


def test_many_jobs_per_launch_at_100_prb_with_sync_and_pbch_subframes():
    """cfg3, 20 subframes from TTI 0 (subframes 0, 5, 10, 15 bring the PSS / SSS / PBCH masks), random CFI: rows of several jobs in flight, TM2 / TM3 / TM4
    up to 256QAM, grants from 4 to 40 PRBs"""
    kw = dict(n_rnti=20, cfi=0)
    dl = _downlink("cfg3", 20, 1, **kw)
    assert {p["format"] for _, p in dl} >= {FMT1A, FMT1, FMT2A, FMT2}
    assert min(p["nof_prb"] for _, p in dl) <= 8 and max(p["nof_prb"] for _, p in dl) >= 24
    assert any(sf == 0 for sf, _ in dl) and any(sf == 5 for sf, _ in dl)
    assert {p["mod"] for _, p in dl} == {2, 4, 6, 8}
    _run("cfg3", 20, seed=1, batch=20, update_meta_period=10, **kw)


@pytest.mark.parametrize("seed,over", [(5, dict(nof_prb=6, cfi=3, dl_min=1, dl_max=1, n_rnti=2)), (6, dict(nof_prb=15, cfi=2, dl_min=1, dl_max=2, n_rnti=3))])
def test_jobs_with_fewer_rows_than_a_workgroup_and_pbch_over_the_whole_band(seed, over):
    dl = _downlink("small", 10, seed, **over)
    assert any(sf == 0 for sf, _ in dl) and any(sf == 5 for sf, _ in dl)
    assert min(p["nof_prb"] for _, p in dl) * (14 - 2) < 16 * 4   # a job of a few work items, the last one partly filled
    _run("small", 10, seed=seed, batch=10, **over)


def test_four_ports_sfbc_fstd_lone_elements_and_odd_counts_per_prb():
    dl = _downlink("small", 12, 12, nof_ports=4)
    assert {p["format"] for _, p in dl} == {FMT1A, FMT1} and any(sf == 0 for sf, _ in dl) and any(sf == 5 for sf, _ in dl)
    _run("small", 12, seed=12, batch=12, nof_ports=4)


def test_extended_cp_twelve_symbols():
    dl = _downlink("small", 12, 31, cp=1)
    assert any(sf == 0 for sf, _ in dl) and any(sf == 5 for sf, _ in dl) and len(dl) > 20
    _run("small", 12, seed=31, batch=12, cp=1)


def test_full_band_two_codewords_row_groups_beyond_one_bytes_worth_of_prbs():
    """one UE over all 100 PRBs, two codewords of 256QAM: 100 x (14 - l0) rows, about 1 300 - row groups 0 .. 80 of one job"""
    kw = dict(n_rnti=1, dl_min=1, dl_max=1, ul_min=0, ul_max=0, mix_tm3_pct=100, mix_tm4_pct=0, pct_256qam=100, mcs_min=26, mcs_max=27, snr_db=40.0,
              rar_period=0, paging_period=0)
    dl = _downlink("cfg3", 3, 41, **kw)
    assert dl and all(p["nof_prb"] == 100 and p["format"] == FMT2A and p["mod"] == 8 for _, p in dl) and {p["tb"] for _, p in dl} == {0, 1}
    _run("cfg3", 3, seed=41, batch=3, **kw)

"""k_rm and k_turbo behind the uplink entry at chosen code blocks (ul_sweep_cases.py; what the plans hold is asserted in test_ul_sweep_plan.py): all 188 turbo block
sizes at gains where the decoder iterates, the same lowered until many blocks fail, the regimes of the rate de-matcher, and one-block calls at the smallest and
the largest size.  Per grant and per code block against the CPU oracle, everything exact: uplink grid, soft bits, the de-rate-matched streams k_rm wrote
(Phy.tap_ul_cbs), the block's verdict and iteration count, the grant's verdict / iteration count / SNR estimate, the payload."""
import time

import numpy as np
import pytest

import ltesniffer_amd as la
from ul_sweep_cases import CELL_ID, CYCLIC_SHIFT, DELTA_SS, NPRB, evaluated

pytestmark = pytest.mark.gpu


def _run(name):
    call, iq, payloads, grids, ores = evaluated(name)
    phy = la.Phy(nof_rx_antennas=1)
    assert phy.setCell(NPRB, 1, CELL_ID) and phy.setUlConfig(CYCLIC_SHIFT, DELTA_SS, 0, 0, 0)
    t0 = time.perf_counter()
    res = phy.pusch_decode(iq, call["tti0"], call["grants"])
    t_gpu = time.perf_counter() - t0
    for sf in range(call["nsf"]):
        assert np.array_equal(phy.tap_ul_grid(sf).reshape(-1).view(np.uint32), grids[sf].view(np.uint32)), (name, sf)
    n_cb = n_ok = n_it = 0
    for i, (g, pl, r, o) in enumerate(zip(call["grants"], payloads, res, ores)):
        assert np.array_equal(phy.tap_ul_llr(i, o["e"].size), o["e"]), (name, i, g)
        cbs = phy.tap_ul_cbs(i)
        assert [(c["K"], c["F"], c["E"], c["rv"]) for c in cbs] == [(b["K"], b["F"], b["E"], b["rv"]) for b in o["blocks"]], (name, i, g)
        for q, (c, b) in enumerate(zip(cbs, o["blocks"])):
            key = (name, i, q, b["K"], b["F"], b["E"], b["rv"], b["off"] % 8)
            if not np.array_equal(c["d3"], b["d3"]):
                d = np.argwhere(c["d3"] != b["d3"])
                raise AssertionError("k_rm differs from the oracle at %s: %d values, first [stream, position] %s: %d vs %d" %
                                     (key, len(d), d[0].tolist(), c["d3"][tuple(d[0])], b["d3"][tuple(d[0])]))
            assert (c["ok"], c["iters"]) == (b["ok"], b["iters"]), key
            n_cb += 1
            n_it += b["iters"]
        assert r["crc_ok"] == o["crc"] and r["iterations"] == o["iters"], (name, i, g, r["crc_ok"], r["iterations"], o["crc"], o["iters"])
        assert np.float32(r["snr_db"]).view(np.uint32) == o["snr_bits"], (name, i, g)
        if o["crc"]:
            assert r["payload"] == o["payload"] == pl, (name, i, g)
            n_ok += 1
    phy.close()
    print("%s: %d subframes, %d grants, %d code blocks (%d oracle iterations), %d transport blocks passed; pusch_decode took %.3f s" %
          (name, call["nsf"], len(call["grants"]), n_cb, n_it, n_ok, t_gpu))
    return n_cb, n_ok


def test_every_turbo_block_size_at_gains_where_the_decoder_iterates():
    n_cb, n_ok = _run("A")
    assert n_cb == n_ok == 188


def test_every_turbo_block_size_with_the_gains_lowered():
    n_cb, n_ok = _run("A-low")
    assert n_cb == 188 and 30 <= n_ok <= 188 - 30      # blocks that run into the iteration limit, and blocks that still pass


def test_regimes_of_the_rate_de_matcher():
    n_cb, n_ok = _run("B")
    assert n_cb >= 50 and n_ok >= 30


@pytest.mark.parametrize("K", [40, 6144])
def test_a_call_of_one_block_at_the_smallest_and_the_largest_size(K):
    assert _run("K%d" % K) == (1, 1)

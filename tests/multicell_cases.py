"""The captures of the multi-cell search tests (tests/test_multicell_model.py on the CPU, tests/test_gpu_multicell.py on the GPU): cell A alone, A plus a second
cell B at another timing / root / both / neither, noise.  Built once per process with the synthetic transmitter and shared."""
import functools

import numpy as np

from lsn_testlib import scenario, sync_capture

NOF_PRB, N, PERIODS = 25, 512, 8
W5, SFLEN = 75 * N, 15 * N
START_TTI = 773
CELL_A = dict(cell_id=301, seed=5, lead=1234, cfo_hz=900.0)
# B: another timing with the same root / with another root, 40 samples beside A with the same root, another root at A's timing
GEOMETRIES = [(304, 9000), (130, 30000), (304, 1274), (302, 1234)]
AMPLITUDES_DB = [0.0, -3.0, -6.0]
WEAK_DB = [-10.0, -14.0]
SHARED = (304, 1234)   # the same root at the same timing as A


@functools.lru_cache(maxsize=None)
def one_cell(cell_id, seed, lead, cfo_hz):
    sc = scenario("small", seed=seed, start_tti=START_TTI, nof_prb=NOF_PRB, cell_id=cell_id, cfo_hz=cfo_hz)
    x, first_tti = sync_capture(sc, lead, PERIODS)
    assert first_tti == START_TTI
    x.setflags(write=False)
    return x


def cell_a():
    return one_cell(CELL_A["cell_id"], CELL_A["seed"], CELL_A["lead"], CELL_A["cfo_hz"])


@functools.lru_cache(maxsize=None)
def two_cells(cell_b, lead_b, amp_db):
    """A + 10^(amp_db / 20) B -> complex64 (read-only)"""
    a, b = cell_a(), one_cell(cell_b, 6, lead_b, -400.0)
    n = min(len(a), len(b))
    x = (a[:n] + np.float32(10.0 ** (amp_db / 20.0)) * b[:n]).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def noise(n=(PERIODS + 1) * W5 + N, seed=3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    x.setflags(write=False)
    return x


def timing(lead, first_tti=START_TTI):
    """(sf_start, sf_idx) of a cell whose subframe first_tti starts at sample lead: the first subframe 0 / 5 boundary in the buffer (tests/test_sync_oracle.py)"""
    k = next(k for k in range(10) if (first_tti + k) % 5 == 0)
    start = (lead + k * SFLEN) % W5
    return start, (first_tti + (start - lead) // SFLEN) % 10


def transmitted(cell_b=None, lead_b=None):
    """cell id -> (sf_start, sf_idx) of what is on the air"""
    t = {CELL_A["cell_id"]: timing(CELL_A["lead"])}
    if cell_b is not None:
        t[cell_b] = timing(lead_b)
    return t

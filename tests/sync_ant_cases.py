"""The captures of the tests of the cell search over all antennas (tests/test_sync_ant_model.py on the CPU, tests/test_gpu_sync_ant.py on the GPU; DESIGN.md
section 3.1r): one cell from the synthetic transmitter (lsn_testlib.sync_capture, as tests/test_gpu_sync.py builds its own) seen by two antennas through chosen
channel gains, with independent receiver noise per antenna; and the two-antenna recording for the carrier scan with one carrier missing per antenna.  Built once per
process, shared, read-only."""
import functools
import math

import numpy as np

from lsn_testlib import scenario, sync_capture

NOF_PRB, N = 6, 128
W5, SFLEN = 75 * N, 15 * N
START_TTI = 10 * 77 + 3
LEAD = 777
SNR_DB = 10.0
OPPOSITE_SEED, FADED_SEED = 41, 42
# the SSS case (found by test_sync_ant_model.sss_candidates: the first of at most 200 (snr, seed) candidates at falling SNR where each antenna's own SSS decision
# is wrong or ambiguous (best / second < 1.2) and the combined one is right and not ambiguous): (snr_db, seed)
SSS_CASE = (-7.0, 19)


@functools.lru_cache(maxsize=None)
def clean_cell(cell_id=77, cp=0, nof_prb=NOF_PRB, periods=2, lead=LEAD, cfo_hz=700.0):
    """one antenna of a cell at 40 dB SNR behind `lead` samples of weak noise -> complex64, read-only"""
    sc = scenario("small", seed=5, start_tti=START_TTI, nof_prb=nof_prb, cell_id=cell_id, cp=cp, cfo_hz=cfo_hz, snr_db=40.0, nof_rx=1, nof_ports=1)
    x, first_tti = sync_capture(sc, lead, periods)
    assert first_tti == START_TTI
    x.setflags(write=False)
    return x


def timing(lead=LEAD, n=N):
    """(sf_start, sf_idx): the capture starts `lead` samples in front of subframe 3, so the first subframe 0 / 5 boundary is subframe 5, two subframes on"""
    return lead + 2 * 15 * n, 5


def noise_like(x, snr_db, seed, lead=LEAD):
    """white noise snr_db under the mean power of the cell's part of x"""
    rng = np.random.default_rng(seed)
    power = float(np.mean(np.abs(x[lead:]) ** 2))
    s = math.sqrt(0.5 * power * 10.0 ** (-snr_db / 10.0))
    return s * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))


@functools.lru_cache(maxsize=None)
def two_antennas(gains, snr_db=SNR_DB, seed=1, **kw):
    """x [2][n] complex64: antenna a = gains[a] * cell + its own noise, snr_db under the cell's power (a gain of 0: noise only)"""
    c = clean_cell(**kw).astype(np.complex128)
    lead = kw.get("lead", LEAD)
    x = np.stack([g * c + noise_like(c, snr_db, 1000 * seed + a, lead) for a, g in enumerate(gains)]).astype(np.complex64)
    x.setflags(write=False)
    return x


def opposite():
    """the same cell with channel gains +1 and -1: the sum of the antennas holds no cell at all"""
    return two_antennas((1.0, -1.0), SNR_DB, OPPOSITE_SEED)


def faded():
    """antenna 0 is noise only, antenna 1 has the cell"""
    return two_antennas((0.0, 1.0), SNR_DB, FADED_SEED)


def sss_case(snr_db, seed):
    return two_antennas((1.0, 1j), snr_db, seed)


@functools.lru_cache(maxsize=None)
def noise(A, P, seed, n=N):
    rng = np.random.default_rng(seed)
    m = (P + 1) * 75 * n + n
    return (rng.standard_normal((A, m)) + 1j * rng.standard_normal((A, m))).astype(np.complex64)


# ---- the carrier scan: a two-antenna 7.68 MS/s head, carrier A (+1.5 MHz, cell 77, extended CP) absent from antenna 1, carrier B (-1.5 MHz, cell 301) absent
# from antenna 0 ----
RATE_SCAN = 7.68e6
SCAN_CARRIERS = [(dict(cell_id=77, cp=1), 1.5e6, 700), (dict(cell_id=301, cp=0), -1.5e6, 2500)]


@functools.lru_cache(maxsize=None)
def scan_recording():
    """-> (x complex64 [n][2] (sample, antenna), [dict(f_hz, cell_id, cp, antenna)]): each carrier a 6-block sync_capture brought from 1.92 to 7.68 MS/s
    (resample_cases.fft_convert) and moved to its offset (ddc_cases.carrier), on ONE antenna; white noise 20 dB under a carrier's power on both"""
    from ddc_cases import carrier
    from resample_cases import fft_convert
    parts = []
    for over, f0, lead in SCAN_CARRIERS:
        sc = scenario("small", seed=5, start_tti=START_TTI, nof_prb=6, **over)
        x, _ = sync_capture(sc, lead, 3)
        parts.append(fft_convert(x, 4, 1))
    n = min(len(p) for p in parts)
    rng = np.random.default_rng(23)
    power = float(np.mean(np.abs(parts[0][:n]) ** 2))
    x = (rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))) * math.sqrt(0.5 * power * 0.01)
    truth = []
    for ant, (y, (over, f0, lead)) in enumerate(zip(parts, SCAN_CARRIERS)):
        x[:, ant] += y[:n] * carrier(n, f0, RATE_SCAN)
        truth.append(dict(f_hz=f0, cell_id=over["cell_id"], cp=over["cp"], antenna=ant))
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x, truth

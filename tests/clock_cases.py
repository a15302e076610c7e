"""Inputs of the sample-clock tests (CPU and GPU): a PSS train synthesised in continuous time at a drifted sample clock - exact, no resampling
filter is involved - and the decoded streams of resample_cases recorded by a clock that is off."""
import functools

import numpy as np

from clock_model import SYMBOL_SZ, pss_sequence

PRB_OF_N = {128: 6, 256: 15, 384: 25, 512: 25, 768: 50, 1024: 50, 1536: 75, 2048: 100}

# name -> (N, periods, eps, snr_db, cfo_hz, blanked periods): the accuracy cases of the issue (three rounds at 120 periods: 8 -> 32 -> 120)
TRAINS = {
    "plus_200ppm": (128, 120, 200e-6, 30.0, 0.0, ()),
    "minus_200ppm": (128, 120, -200e-6, 30.0, 0.0, ()),
    "plus_3ppm": (128, 120, 3e-6, 30.0, 0.0, ()),
    "plus_20ppm_10db_cfo_blanked": (128, 120, 20e-6, 10.0, 2000.0, tuple(range(40, 50))),
}


def pss_train(N, periods, eps, snr_db, cfo_hz=0.0, blank=(), n_id_2=1, seed=1, u0=1234.3, loaded=True):
    """A recording of `periods` 5 ms periods made by a clock that runs at fs (1 + eps): sample n is taken at t = n / (fs (1 + eps)).  Every period carries, from
    u0 + q 75 N nominal samples on, the useful part of a PSS symbol; that symbol (with its cyclic prefix) and the fully loaded symbols in front of and behind it
    are evaluated at the sampling instants as sum_k X_k exp(2 pi j 15 kHz k (t - t_symbol)).  Loaded symbols have unit power; receiver noise of 10^(-snr_db / 10)
    fills everything, the space between the bursts included; periods in `blank` carry noise only; loaded = False leaves the two neighbour symbols out (a timing
    probe's long recording).  The whole recording is turned by exp(2 pi j cfo_hz t).
    -> (x complex64, dict(p0 = true position of occurrence 0, pss_pos = the integer next to it, n_id_2, N, eps, W5))"""
    rng = np.random.default_rng(seed)
    W5, cp = 75 * N, 144 * N // 2048
    nre = 6 * PRB_OF_N[N]                       # occupied carriers on each side of DC
    total = int(np.ceil(u0)) + periods * W5
    sigma = 10.0 ** (-snr_db / 20.0)
    x = (rng.standard_normal(total) + 1j * rng.standard_normal(total)) * (sigma / np.sqrt(2.0))
    amp = 1.0 / np.sqrt(2.0 * nre)
    k_all = np.concatenate([np.arange(-nre, 0), np.arange(1, nre + 1)]).astype(np.float64)
    k_pss = np.concatenate([np.arange(-31, 0), np.arange(1, 32)]).astype(np.float64)
    d = pss_sequence(n_id_2)
    for q in range(periods):
        if q in blank:
            continue
        s = u0 + q * W5                         # useful part of the PSS symbol, nominal samples
        for start, kk, X in ((s - cp - N - cp, k_all, None), (s - cp, k_pss, d), (s + N, k_all, None)):
            if X is None and not loaded:
                continue
            if X is None:
                X = (rng.choice([-1.0, 1.0], len(kk)) + 1j * rng.choice([-1.0, 1.0], len(kk))) / np.sqrt(2.0)
            n_lo, n_hi = int(np.ceil(start * (1.0 + eps))), int(np.ceil((start + cp + N) * (1.0 + eps)))
            n_lo, n_hi = max(n_lo, 0), min(n_hi, total)
            u = np.arange(n_lo, n_hi, dtype=np.float64) / (1.0 + eps) - (start + cp)   # nominal samples from the start of the symbol's useful part
            x[n_lo:n_hi] += amp * (np.exp(2j * np.pi * np.outer(u, kk) / N) @ X)
    if cfo_hz:
        x *= np.exp(2j * np.pi * cfo_hz * np.arange(total) / (15000.0 * N * (1.0 + eps)))
    p0 = u0 * (1.0 + eps)
    return x.astype(np.complex64), dict(p0=p0, pss_pos=int(round(p0)), n_id_2=n_id_2, N=N, eps=eps, W5=W5)


@functools.lru_cache(maxsize=None)
def train(name):
    N, periods, eps, snr_db, cfo_hz, blank = TRAINS[name]
    x, info = pss_train(N, periods, eps, snr_db, cfo_hz, blank)
    info.update(cfo_hz=cfo_hz, blank=blank, periods=periods)
    x.setflags(write=False)
    return x, info


def end_error(eps_hat, eps, nof_samples):
    """the misalignment at the end of the recording that the estimate leaves, in samples"""
    return abs(eps_hat - eps) * nof_samples


@functools.lru_cache(maxsize=None)
def drifted_capture(case):
    """resample_cases.foreign_capture of a ppm case, read as the issue reads it: a recording at the NOMINAL rate whose clock is off -> (sc, tti0, oracle records,
    options, nominal rate, eps, file samples [sample][antenna] complex128 (sample LEAD = first sample of the stream))"""
    from resample_cases import foreign_capture
    sc, tti0, orecs, otrace, opt, rate_in, native, f = foreign_capture(case)
    return sc, tti0, orecs, opt, native, rate_in / native - 1.0, f


def symbol_sz(nof_prb, rates=0):
    return SYMBOL_SZ[(nof_prb, rates)]

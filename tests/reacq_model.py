"""float64 restatement of a stream's re-acquisition (lsn_stream_reacquire, k_pss_acquire), written from the definition in include/ltesniffer_amd.h / DESIGN.md
section 3.1k: the search metric over a half frame of lags, the decision, and the rule that says when a search is due and when its result moves the position.
Shares no code with the library."""
import numpy as np

from track_model import lag_spacing, pss_index

SPAN_SUBFRAMES = 6      # the span of a search: segment h and one subframe more
FAR = 8                 # lags: `far` is the largest value further than this from the maximum, circularly
MIN_RATIO = 3.0         # the default: the geometric mean of the ratio on noise (1.86) and with the cell present (5.1)
DELAY = 3               # the search of segment h is taken in on entering segment h + 3


def nof_lags(N):
    return 75 * N // lag_spacing(N)


def metric(x, r, d, with_bound=False):
    """x: [6][antenna][15 N] (the block-buffer layout: the subframes of one antenna follow each other in time), r: the replica [N] -> C[75 N / d] in float64,
    C_i = sum_a |sum_k x_a[i d + k] conj r[k]|^2 / sum_a sum_k |x_a[i d + k]|^2, 0 when the denominator is 0.  with_bound: also the largest error a float32
    evaluation can make per value - track_model.corr13's bound: (N + 3) 2^-24 times the sum of magnitudes of each dot product, through the square and the quotient"""
    x = np.asarray(x)
    r = np.asarray(r).astype(np.complex128)
    N = len(r)
    assert x.ndim == 3 and x.shape[0] == SPAN_SUBFRAMES and x.shape[2] == 15 * N
    n = 75 * N // d
    u = 2.0 ** -24
    g = (N + 3) * u
    num, den, dnum = np.zeros(n), np.zeros(n), np.zeros(n)
    rr, ri = r.real, r.imag
    arr, ari = np.abs(rr), np.abs(ri)
    for a in range(x.shape[1]):
        t = x[:, a, :].reshape(-1).astype(np.complex128)          # 90 N samples in time
        win = np.lib.stride_tricks.sliding_window_view(t, N)[::d][:n]
        for c0 in range(0, n, 1200):
            v = win[c0:c0 + 1200]
            vr, vi = v.real, v.imag
            s_re, s_im = vr @ rr + vi @ ri, vi @ rr - vr @ ri
            num[c0:c0 + 1200] += s_re ** 2 + s_im ** 2
            den[c0:c0 + 1200] += np.sum(vr ** 2 + vi ** 2, axis=1)
            if with_bound:
                m_re, m_im = np.abs(vr) @ arr + np.abs(vi) @ ari, np.abs(vi) @ arr + np.abs(vr) @ ari
                dnum[c0:c0 + 1200] += 2.0 * (np.abs(s_re) * g * m_re + np.abs(s_im) * g * m_im) + (g * m_re) ** 2 + (g * m_im) ** 2
    ok = den > 0.0
    C = np.where(ok, num / np.where(ok, den, 1.0), 0.0)
    if not with_bound:
        return C
    dnum = dnum + 4.0 * u * num
    B = np.where(ok, (dnum + num * (g + u)) / (np.where(ok, den, 1.0) * (1.0 - g)) + u * C, 0.0)
    return C, B


def far_value(C, i):
    """the largest C_j whose circular distance from i is above FAR lags"""
    n = len(C)
    j = np.arange(n)
    dist = np.minimum((j - i) % n, (i - j) % n)
    return float(np.max(C[dist > FAR]))


def decide(C, d, N, min_ratio=MIN_RATIO, history_mean=None):
    """-> (accepted, o in output samples, peak, peak / far).  i* the first maximum; accepted when peak > 0, peak >= min_ratio far and peak >= 0.25 history_mean
    (None: an empty history accepts); o = ((i* d - p + W5 / 2) mod W5) - W5 / 2: the nearest PSS"""
    C = np.asarray(C, dtype=np.float64)
    W5, p = 75 * N, pss_index(N)
    assert len(C) * d == W5
    i = int(np.argmax(C))
    peak = float(C[i])
    far = far_value(C, i)
    ok = peak > 0.0 and peak >= min_ratio * far and (history_mean is None or peak >= 0.25 * history_mean)
    o = ((i * d - p + W5 // 2) % W5) - W5 // 2
    ratio = peak / far if far > 0.0 else (float("inf") if peak > 0.0 else 0.0)
    return ok, o, peak, ratio


class Rule:
    """when a search is due and when it is taken in, for one cell.  entered(h, invalid_run) is called on entering segment h, after the loop step that consumed the
    measurement of segment h - 2, with result(h0) a callable that runs the search of segment h0 -> decide()'s tuple, or None when it could not be launched.
    -> (jump in output samples or None, search due for this segment)"""

    def __init__(self, after):
        self.after, self.in_flight, self.log = after, None, []

    def entered(self, h, invalid_run, result):
        jump = None
        if self.in_flight is not None and h == self.in_flight + DELAY:
            res = result(self.in_flight)
            self.log.append((self.in_flight, res))
            if res is not None and res[0]:
                jump = res[1]
                invalid_run = 0
            self.in_flight = None
        if self.in_flight is None and invalid_run >= self.after:
            self.in_flight = h
        return jump, invalid_run, self.in_flight == h

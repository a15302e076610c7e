"""Float64 model of the product's polyphase resampler, written from the definition in DESIGN.md section 3.1b (not from the kernel or its table code).

Positions: output sample m sits at input position P0 + m D, integers in 64.64 fixed point (Python integers here):
    D  = floor(rate_in / rate_out * 2^64 + 1/2), the quotient of the two doubles taken exactly,
    P0 = first_sample * 2^64 + floor(first_frac * 2^64).
Filter: with rho = max(1, rate_in / rate_out), B the pass-band edge and A = 80 dB,
    beta = 0.1102 (A - 8.7),   width = (min(rate_in, rate_out) - 2 B) / rate_in,   T = max(4, 2 ceil(((A - 7.95) / (14.36 width) + 1) / 2)),
    h(t) = sinc(t / rho) / rho * I0(beta sqrt(1 - (2 t / T)^2)) / I0(beta)   for |t| <= T / 2, else 0   (t in input samples).
Bank: H[p][j] = h(j - T/2 + 1 - p / 512), p = 0 .. 512, j = 0 .. T - 1.  For a position with integer part n0 and fraction F (64 bits):
    p = the top 9 bits of F,   f = the next 24 bits / 2^24,   c_j = H[p][j] + f (H[p + 1][j] - H[p][j]),
    y[m] = sum_j c_j x[n0 - T/2 + 1 + j],   x[n] = 0 for n < 0.
"""
import math
from fractions import Fraction

import numpy as np

ATTEN_DB = 80.0
PHASES = 512
MAX_TAPS = 192


def passband_hz(nof_prb):
    return 15000.0 * (6 * nof_prb + 1)


class Plan:
    def __init__(self, rate_in, rate_out, passband, first_sample=0, first_frac=0.0):
        rate_in, rate_out = float(rate_in), float(rate_out)
        self.rate_in, self.rate_out = rate_in, rate_out
        self.step = int((2 * Fraction(rate_in) / Fraction(rate_out) * 2 ** 64 + 1) // 2)
        self.start = (int(first_sample) << 64) + int(Fraction(first_frac) * 2 ** 64)
        self.rho = max(1.0, rate_in / rate_out)
        width = (min(rate_in, rate_out) - 2.0 * passband) / rate_in
        if not width > 0 or rate_in > 4 * rate_out:
            raise ValueError("outside the accepted range")
        want = (ATTEN_DB - 7.95) / (14.36 * width) + 1.0
        if want > MAX_TAPS:
            raise ValueError("outside the accepted range")
        self.taps = T = max(4, 2 * int(math.ceil(want / 2.0)))
        beta = 0.1102 * (ATTEN_DB - 8.7)
        t = np.arange(T)[None, :] - T / 2 + 1 - np.arange(PHASES + 1)[:, None] / PHASES
        u = np.clip(1.0 - (2.0 * t / T) ** 2, 0.0, None)
        self.H = np.sinc(t / self.rho) / self.rho * np.i0(beta * np.sqrt(u)) / np.i0(beta)
        self.H[np.abs(t) > T / 2] = 0.0

    def position(self, m):
        return self.start + int(m) * self.step

    def span(self, m0, n):
        """input samples [lo, hi) read by outputs m0 .. m0 + n - 1"""
        return (self.position(m0) >> 64) - self.taps // 2 + 1, (self.position(m0 + max(n, 1) - 1) >> 64) + self.taps // 2 + 1

    def max_out(self, in_end):
        """number of outputs m = 0, 1, .. whose taps all lie in front of input sample in_end"""
        lim = (in_end - self.taps // 2) << 64
        return 0 if self.start >= lim or in_end <= self.taps // 2 else (lim - 1 - self.start) // self.step + 1

    def phases(self, m0, n):
        pos = [self.start + m * self.step for m in range(m0, m0 + n)]
        n0 = np.array([p >> 64 for p in pos], dtype=np.int64)
        ph = np.array([(p >> 55) & 511 for p in pos], dtype=np.int64)
        f = np.array([(p >> 31) & 0xFFFFFF for p in pos], dtype=np.float64) / 2.0 ** 24
        return pos, n0, ph, f

    def apply(self, x, m0, n, in_base=0, with_bound=False):
        """x[sample] or x[sample][antenna], x[0] = input sample in_base -> y[n] / y[n][antenna] complex128 (and sum_j |c_j| |x_j| per output)"""
        x = np.asarray(x)
        x = x.astype(np.complex128)
        T = self.taps
        y = np.zeros((n,) + x.shape[1:], dtype=np.complex128)
        bound = np.zeros((n,) + x.shape[1:], dtype=np.float64)
        for c0 in range(0, n, 32768):
            c1 = min(n, c0 + 32768)
            _, n0, ph, f = self.phases(m0 + c0, c1 - c0)
            c = self.H[ph] + f[:, None] * (self.H[ph + 1] - self.H[ph])            # [n, T]
            idx = n0[:, None] - T // 2 + 1 + np.arange(T)[None, :]                # absolute input sample
            k = idx - in_base
            assert np.all((idx < 0) | ((k >= 0) & (k < x.shape[0]))), "the input does not hold what these outputs read"
            xs = x[np.clip(k, 0, x.shape[0] - 1)]
            xs[idx < 0] = 0.0
            cc = c.reshape(c.shape + (1,) * (x.ndim - 1))
            y[c0:c1] = np.sum(cc * xs, axis=1)
            if with_bound:
                bound[c0:c1] = np.sum(np.abs(cc) * np.abs(xs), axis=1)
        return (y, bound) if with_bound else y

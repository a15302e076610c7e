"""Float64 model of the channel filter, stage 1 in front of the resampler, written from the definition in DESIGN.md section 3.1f (not from the kernel or
the library's design code).

With R the recording's rate, B the pass-band edge, S the stop band, A = 80 and beta = 0.1102 (A - 8.7):
    width = (S - B) / R,   L = ceil((A - 7.95) / (14.36 width) / 2),   fc = (B + S) / (2 R),
    g[j]  = 2 fc sinc(2 fc j) I0(beta sqrt(1 - (j / (L + 1))^2)) / I0(beta),  j = -L .. L, rounded to float32 once,
    xm[n] = x[n] exp(-2 pi j (n W mod 2^64) / 2^64)  (ddc_cases.mix: exact integer phase; W = 0: no mixer),  xm[n] = 0 for n < 0,
    y1[n] = sum over k = n - L .. n + L of g[n - k] xm[k].
Stage 2 is resample_model.Plan of the same rate pair, pass band and start, reading y1 (zeros in front of sample 0)."""
import math

import numpy as np

from ddc_cases import mix, tuning_word

ATTEN_DB = 80.0
MAX_L = 512


class Design:
    def __init__(self, rate_in, passband, stopband):
        R, B, S = float(rate_in), float(passband), float(stopband)
        if not (math.isfinite(S) and B < S <= R / 2):
            raise ValueError("outside the accepted range")
        width = (S - B) / R
        self.L = L = int(math.ceil((ATTEN_DB - 7.95) / (14.36 * width) / 2.0))
        if L > MAX_L:
            raise ValueError("outside the accepted range")
        self.rate_in, self.passband, self.stopband = R, B, S
        self.fc = fc = (B + S) / (2.0 * R)
        beta = 0.1102 * (ATTEN_DB - 8.7)
        j = np.arange(-L, L + 1, dtype=np.float64)
        g = 2.0 * fc * np.sinc(2.0 * fc * j) * np.i0(beta * np.sqrt(1.0 - (j / (L + 1)) ** 2)) / np.i0(beta)
        self.g32 = g.astype(np.float32)
        self.g = self.g32.astype(np.float64)      # the taps the product multiplies with

    def span(self, n0, n):
        """input samples [lo, hi) that y1[n0 .. n0 + n - 1] read"""
        return n0 - self.L, n0 + n + self.L

    def max_out(self, in_end):
        """number of y1[n], n = 0, 1, .., whose input lies in front of sample in_end"""
        return max(in_end - self.L, 0)

    def response(self, f_hz):
        """gain of the float32 taps at f_hz (array), relative to the carrier the mixer moved to 0"""
        j = np.arange(-self.L, self.L + 1, dtype=np.float64)
        return np.array([np.sum(self.g * np.exp(-2j * np.pi * f / self.rate_in * j)) for f in np.atleast_1d(f_hz)])

    def apply(self, x, in_base, n0, n, center_offset_hz=0.0, with_bound=False):
        """x[sample] or x[sample][antenna], x[0] = sample in_base of the recording -> y1[n0 .. n0 + n - 1] complex128, same trailing shape (and sum |g| |xm| per
        output).  Samples in front of sample 0 are zeros; every other sample the outputs read must be in x"""
        x = np.asarray(x)
        lo, hi = self.span(n0, n)
        need_lo = max(lo, 0)
        assert need_lo >= in_base and hi <= in_base + x.shape[0], "the input does not hold what these outputs read"
        seg = x[need_lo - in_base:hi - in_base]
        W = tuning_word(center_offset_hz, self.rate_in) if center_offset_hz != 0.0 else 0
        xm = mix(seg, need_lo, W) if W else seg.astype(np.complex128)
        flat = xm.reshape(xm.shape[0], -1)
        pad = np.zeros((need_lo - lo, flat.shape[1]), dtype=np.complex128)
        flat = np.concatenate([pad, flat])                       # flat[0] = sample lo
        y = np.stack([np.convolve(flat[:, a], self.g, mode="valid") for a in range(flat.shape[1])], axis=1)
        assert y.shape[0] == n
        y = y.reshape((n,) + x.shape[1:])
        if not with_bound:
            return y
        b = np.stack([np.convolve(np.abs(flat[:, a]), np.abs(self.g), mode="valid") for a in range(flat.shape[1])], axis=1)
        return y, b.reshape((n,) + x.shape[1:])


def two_stage(design, plan, x, center_offset_hz, n_out, in_end=None):
    """the float64 model of a filtered replay of the recording x (x[0] = sample 0): stage 1 over what stage 2 reads, then plan (resample_model.Plan of the
    same start, no offset) -> y[n_out] / y[n_out][antenna]"""
    lo, hi = plan.span(0, n_out)
    lo = max(lo, 0)
    assert hi + design.L <= (len(x) if in_end is None else in_end)
    y1 = design.apply(x, 0, lo, hi - lo, center_offset_hz)
    return plan.apply(y1, 0, n_out, in_base=lo)

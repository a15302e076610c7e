"""float64 restatement of a stream's timing loop (lsn_stream_track, k_pss_timing), written from the definition in include/ltesniffer_amd.h / DESIGN.md section
3.1h: the 13 values of the detector, the observation, the peak test, the proportional-integral loop and the phase-domain plant it is simulated against.
Shares no code with the library."""
import math

import numpy as np

G, LAGS, SEG_SUBFRAMES, DELAY = 6, 13, 5, 2
KP, KI, MAX_PPM, LOST_AFTER = 0.25, 1.0 / 32.0, 100.0, 40


def lag_spacing(N):
    return max(1, N // 128)


def pss_index(N):
    """first useful sample of the PSS symbol inside a subframe 0 / 5: symbol 6 of slot 0 (normal prefix: 160 + 6 144 + 6 2048 at N = 2048), symbol 5 with the
    extended prefix (6 512 + 5 2048) - 13 N / 2 either way"""
    return 13 * N // 2


def corr13(x, p, r, d, with_bound=False):
    """x: [antenna][samples] of one subframe, r: the replica [N] -> C[13] in float64 (the inputs are float32 values: the sums are exact to float64's rounding).
    with_bound: also the largest error a float32 evaluation can make per value - (N + 3) 2^-24 times the sum of magnitudes of each dot product, through the
    square and the quotient"""
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    r = np.asarray(r).astype(np.complex128)
    N = len(r)
    u = 2.0 ** -24
    g = (N + 3) * u
    C, B = np.zeros(LAGS), np.zeros(LAGS)
    for j in range(LAGS):
        lo = p + (j - G) * d
        assert lo >= 0 and lo + N <= x.shape[1]
        num = den = dnum = 0.0
        for a in range(x.shape[0]):
            v = x[a, lo:lo + N]
            s = np.sum(v * np.conj(r))
            m_re = float(np.sum(np.abs(v.real * r.real) + np.abs(v.imag * r.imag)))
            m_im = float(np.sum(np.abs(v.imag * r.real) + np.abs(v.real * r.imag)))
            num += abs(s) ** 2
            den += float(np.sum(v.real ** 2 + v.imag ** 2))
            dnum += 2.0 * (abs(s.real) * g * m_re + abs(s.imag) * g * m_im) + (g * m_re) ** 2 + (g * m_im) ** 2
        if den > 0.0:
            C[j] = num / den
            dnum += 4.0 * u * num                       # the squares, their sum, the sum over the antennas
            B[j] = (dnum + num * (g + u)) / (den * (1.0 - g)) + u * C[j]   # the denominator is a sum of positive terms: relative error g; the quotient's rounding
    return (C, B) if with_bound else C


def observe(C, d):
    """-> (geometrically valid, e in output samples, peak): first maximum, interior, parabola through the three values"""
    b = int(np.argmax(C))
    peak = float(C[b])
    if b == 0 or b == LAGS - 1:
        return False, 0.0, peak
    cm, c0, cp = float(C[b - 1]), float(C[b]), float(C[b + 1])
    frac = 0.5 * (cm - cp) / (cm - 2.0 * c0 + cp)
    return True, ((b - 6.0) + frac) * d, peak


class Peaks:
    """peak >= 0.25 mean(the last up to 8 valid peaks); the first one is valid; a valid peak joins the history"""

    def __init__(self):
        self.hist = []

    def accept(self, peak):
        if self.hist:
            s = 0.0
            for v in self.hist:
                s = s + v
            if not peak >= 0.25 * (s / len(self.hist)):
                return False
        self.hist = (self.hist + [peak])[-8:]
        return True


def new_state(initial_ppm=0.0, seglen=1):
    c = initial_ppm * 1e-6 * seglen
    return dict(integrator=c, correction=c, invalid_run=0, lost=0)


def delta_of(c, rate_in, rate_out, seglen):
    """(int) nearbyint(ldexp(rate_in / rate_out, 64) * c / seglen): round half to even, as the default rounding mode"""
    v = math.ldexp(rate_in / rate_out, 64) * c
    return int(round(v / float(seglen)))


def loop_step(state, e, valid, rate_in, rate_out, seglen, kp=KP, ki=KI, max_ppm=MAX_PPM, lost_after=LOST_AFTER):
    """one step -> (new state, step - step_nominal in units of 2^-64 input samples)"""
    lim = max_ppm * 1e-6 * float(seglen)

    def clamp(v):
        return lim if v > lim else (-lim if v < -lim else v)
    s = dict(state)
    if valid:
        cand = clamp(s["integrator"] + ki * e)
        u = kp * e + cand
        if not ((u > lim and e > 0.0) or (u < -lim and e < 0.0)):      # anti-windup: a correction at its limit that e pushes further out holds the integrator
            s["integrator"] = cand
        s["correction"] = clamp(kp * e + s["integrator"])
        s["invalid_run"], s["lost"] = 0, 0
    else:
        s["correction"] = s["integrator"]
        s["invalid_run"] = min(s["invalid_run"] + 1, 0xFFFFFFFF)
        if s["invalid_run"] >= lost_after:
            s["lost"] = 1
    return s, delta_of(s["correction"], rate_in, rate_out, seglen)


def simulate(drift, nseg, seglen, noise=None, valid=None, **gains):
    """the phase-domain plant with the loop's two-segment delay: x[h + 3] = x[h + 2] + drift[h + 2] - c[h], x the timing error in output samples at the PSS of
    segment h (x[0] = 0; segments 0 and 1 run uncorrected: x[1] = drift[0], x[2] = x[1] + drift[1]), c[h] the correction the loop forms from the measurement
    x[h] + noise[h] of segment h.  drift: a number or a sequence (output samples per segment).  -> (x, c, states)"""
    dr = [float(drift)] * (nseg + 3) if np.isscalar(drift) else [float(v) for v in drift]
    x = [0.0] * (nseg + 3)
    x[1] = x[0] + dr[0]
    x[2] = x[1] + dr[1]
    st = new_state()
    cs, states = [], []
    for h in range(nseg):
        ok = True if valid is None else bool(valid[h])
        e = x[h] + (0.0 if noise is None else float(noise[h]))
        st, _ = loop_step(st, e, ok, 1.0, 1.0, seglen, **gains)
        cs.append(st["correction"])
        states.append(st)
        x[h + 3] = x[h + 2] + dr[h + 2] - st["correction"]
    return x[:nseg], cs, states

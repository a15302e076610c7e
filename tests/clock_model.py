"""numpy restatement of the sample-clock estimate (lsn_clock_*), written from the definition in include/ltesniffer_amd.h / DESIGN.md section 3.1c:
the correlation C in float32 with a Python loop over the taps and vector operations over the lags (the kernel's order, one rounding per operation),
observation, plan and fit in float64.  Shares no code with the library."""
import functools
import math

import numpy as np

GUARD, ROUND0, MAX_PERIODS = 4, 8, 4096
ROOTS = (25, 29, 34)
SYMBOL_SZ = {(6, 0): 128, (15, 0): 256, (25, 0): 512, (50, 0): 1024, (75, 0): 1536, (100, 0): 2048,
             (6, 1): 128, (15, 1): 256, (25, 1): 384, (50, 1): 768, (75, 1): 1024, (100, 1): 1536}


def pss_sequence(n_id_2):
    """36.211 6.11.1.1: the 62 values of the Zadoff-Chu sequence on carriers -31..-1, +1..+31 (float64)"""
    d = np.zeros(62, dtype=np.complex128)
    for n in range(62):
        a = n * (n + 1) if n < 31 else (n + 1) * (n + 2)
        ph = -math.pi * ROOTS[n_id_2] * (a % 126) / 63.0
        d[n] = complex(math.cos(ph), math.sin(ph))
    return d


@functools.lru_cache(maxsize=None)
def replica(n_id_2, N, cfo_hz=0.0):
    """the correlator's replica: IDFT of the PSS (its 62 values as float32, as the cell search keeps them) scaled to unit energy, times
    exp(2 pi j cfo_hz k / fs), everything in float64, rounded to float32 once -> complex64 [N]"""
    d = pss_sequence(n_id_2).astype(np.complex64)
    dr, di = [float(v) for v in d.real], [float(v) for v in d.imag]
    bins = [N - 31 + m if m < 31 else m - 30 for m in range(62)]
    sc, fs = 1.0 / math.sqrt(62.0 * N), 15000.0 * N
    out = np.zeros(N, dtype=np.complex64)
    for n in range(N):
        ar = ai = 0.0
        for m in range(62):
            ph = 2.0 * math.pi * float((bins[m] * n) % N) / float(N)
            c, s = math.cos(ph), math.sin(ph)
            ar += dr[m] * c - di[m] * s
            ai += dr[m] * s + di[m] * c
        ar, ai = ar * sc, ai * sc
        if cfo_hz != 0.0:
            ph = 2.0 * math.pi * float(cfo_hz) * float(n) / fs
            c, s = math.cos(ph), math.sin(ph)
            ar, ai = ar * c - ai * s, ar * s + ai * c
        out[n] = np.float32(ar) + 1j * np.float32(ai)
    return out


def corr(x, r, windows):
    """C of every lag of every window [(centre, half_width)] -> list of float32 arrays.  Sums over k in index order, float32, one rounding per operation."""
    x = np.asarray(x, dtype=np.complex64)
    r = np.asarray(r, dtype=np.complex64)
    N = len(r)
    lags = np.concatenate([np.arange(c - h, c + h + 1, dtype=np.int64) for c, h in windows])
    assert lags.min() >= 0 and lags.max() + N <= len(x)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    pr, pi = np.ascontiguousarray(r.real), np.ascontiguousarray(r.imag)
    ar = np.zeros(len(lags), dtype=np.float32)
    ai = np.zeros(len(lags), dtype=np.float32)
    e = np.zeros(len(lags), dtype=np.float32)
    for k in range(N):
        vr, vi = xr[lags + k], xi[lags + k]
        a_r, a_i = pr[k], pi[k]
        e = e + (vr * vr + vi * vi)
        ar = ar + (vr * a_r + vi * a_i)
        ai = ai + (vi * a_r - vr * a_i)
    assert ar.dtype == np.float32 and e.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        C = np.where(e > 0, (ar * ar + ai * ai) / e, np.float32(0.0)).astype(np.float32)
    out, o = [], 0
    for c, h in windows:
        out.append(C[o:o + 2 * h + 1])
        o += 2 * h + 1
    return out


def observe(C, centre, h):
    """-> (valid, pos, peak): first maximum, interior, parabola through the three lags (float64)"""
    b = int(np.argmax(C))
    if b == 0 or b == len(C) - 1:
        return 0, 0.0, float(C[b])
    cm, c0, cp = float(C[b - 1]), float(C[b]), float(C[b + 1])
    return 1, float(centre - h + b) + 0.5 * (cm - cp) / (cm - 2.0 * c0 + cp), c0


def nof_periods(N, pss_pos, nof_samples, max_ppm=200.0, max_periods=0):
    """Q: the periods whose round-0-style window lies inside the samples"""
    W5, Q = 75 * N, 0
    for q in range(max_periods if 0 < max_periods < MAX_PERIODS else MAX_PERIODS):
        c, h = pss_pos + q * W5, GUARD + math.ceil(q * W5 * max_ppm * 1e-6)
        if c - h < 0 or c + h + N > nof_samples:
            break
        Q += 1
    return Q


def schedule(Q):
    """periods per round: 8, 32, 128, ... capped by Q, the last equal to Q"""
    out = [min(Q, ROUND0)]
    while out[-1] < Q:
        out.append(min(Q, 4 * out[-1]))
    return out


def plan(N, pss_pos, nof_samples, rnd, prev=None, max_ppm=200.0, max_periods=0):
    """windows of round rnd -> [(period, centre, half_width)]; prev = the fit of the round before (dict with eps, pss_pos0)"""
    W5, Q = 75 * N, nof_periods(N, pss_pos, nof_samples, max_ppm, max_periods)
    assert Q >= 4
    sched = schedule(Q)
    if rnd >= len(sched):
        return []
    if rnd == 0:
        return [(q, pss_pos + q * W5, GUARD + math.ceil(q * W5 * max_ppm * 1e-6)) for q in range(sched[0])]
    d = sched[rnd - 1] - 1
    return [(q, math.floor(prev["pss_pos0"] + (q * W5) * (1.0 + prev["eps"]) + 0.5), GUARD + -(-q // d)) for q in range(sched[rnd])]


def fit(obs, W5):
    """obs: [(period, valid, pos, peak)] -> dict(found, nof_periods, nof_used, eps, pss_pos0, rms_residual, max_residual)"""
    out = dict(found=0, nof_periods=len(obs), nof_used=0, eps=0.0, pss_pos0=0.0, rms_residual=0.0, max_residual=0.0)
    v = [(q, pos, pk) for q, valid, pos, pk in obs if valid]
    if not v:
        return out
    med = float(np.median(np.array([pk for _, _, pk in v], dtype=np.float64)))
    v = [(q, pos) for q, pos, pk in v if pk >= 0.25 * med]

    def ols(v):
        q = np.array([a for a, _ in v], dtype=np.float64)
        d = np.array([p - a * W5 for a, p in v], dtype=np.float64)   # the drift against the nominal grid: exact, and small
        qm, dm = q.mean(), d.mean()
        sqq = float(np.sum((q - qm) ** 2))
        if not sqq > 0:
            return None
        slope = float(np.sum((q - qm) * (d - dm))) / sqq
        icpt = dm - slope * qm
        return slope, icpt, d - (icpt + slope * q)

    out["nof_used"] = len(v)
    f = ols(v) if len(v) >= 2 else None
    if f is None:
        return out
    v = [o for o, r in zip(v, f[2]) if not abs(r) > 1.0]
    out["nof_used"] = len(v)
    f = ols(v) if len(v) >= 2 else None
    if f is None:
        return out
    slope, icpt, res = f
    out.update(eps=slope / W5, pss_pos0=float(icpt), rms_residual=float(np.sqrt(np.mean(res ** 2))), max_residual=float(np.max(np.abs(res))))
    out["found"] = int(len(v) >= 4 and 2 * len(v) >= len(obs) and out["rms_residual"] <= 0.5)
    return out


def estimate(x, N, n_id_2, pss_pos, cfo_hz=0.0, max_ppm=200.0, max_periods=0, sf_start=0, rep=None):
    """all rounds -> (dict of the last fit + nof_rounds, sample_rate_hz, sf_start; observations of the last round [(period, valid, centre, half_width, pos, peak)])"""
    W5 = 75 * N
    r = replica(n_id_2, N, float(np.float32(cfo_hz))) if rep is None else rep
    prev, res, obs, rnd = None, None, [], 0
    while True:
        w = plan(N, pss_pos, len(x), rnd, prev, max_ppm, max_periods)
        if not w:
            break
        if any(c - h < 0 or c + h + N > len(x) for _, c, h in w):
            res = dict(res or fit([], W5), found=0, nof_rounds=rnd + 1)
            break
        Cs = corr(x, r, [(c, h) for _, c, h in w])
        obs = [(q, c, h) + observe(C, c, h) for (q, c, h), C in zip(w, Cs)]
        res = fit([(q, valid, pos, pk) for q, c, h, valid, pos, pk in obs], W5)
        res["nof_rounds"] = rnd + 1
        if not res["found"]:
            break
        prev = res
        rnd += 1
    if res["found"]:
        d = (pss_pos - sf_start) % W5
        s = res["pss_pos0"] - d * (1.0 + res["eps"])
        while s < 0:
            s += W5 * (1.0 + res["eps"])
        res.update(sample_rate_hz=15000.0 * N * (1.0 + res["eps"]), sf_start=s)
    return res, [(q, valid, c, h, pos, pk) for q, c, h, valid, pos, pk in obs]

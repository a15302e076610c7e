"""float64 restatement of the successive cell search (lsn_cell_search_all), written from that text: the PSS correlation, the
cancellation of an accepted cell's PSS, the lags a cancellation changes, the SSS decision accumulated over all occurrences, the rule of a round, and the float32
error bounds the GPU tests hold the kernels to.  Shares no code with the library; sequences come from the oracle and from clock_model (itself a restatement)."""
import functools
import math

import numpy as np

import clock_model as cm
from lsn_testlib import oracle_sync_api

U = 2.0 ** -24
SYMBOL = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}
THRESHOLD_NEXT, SSS_RATIO_MIN, SHARED_PSS_RATIO, MAX_CELLS = 8.0, 1.5, 0.6, 8


def replica(n_id_2, N, cfo_hz=0.0):
    """unit-energy PSS replica rotated by cfo_hz, rounded to float32 once -> complex64 [N]"""
    return cm.replica(n_id_2, N, float(np.float32(cfo_hz)))


@functools.lru_cache(maxsize=None)
def sss_table(n_id_2):
    """[336][62] of +-1: row h = 2 N_id_1 + (subframe 5)"""
    o = oracle_sync_api()
    t = np.zeros((336, 62), dtype=np.int8)
    for n1 in range(168):
        for h in range(2):
            o.o_sss_seq(n1, n_id_2, h, t[2 * n1 + h].ctypes.data)
    return t.astype(np.float64)


def carrier_bins(N):
    return np.array([N - 31 + m if m < 31 else m - 30 for m in range(62)])


# ---------------- correlation ----------------
def corr_direct(x, reps, N, P, lags):
    """C[root][lag] for the given lags: sum over P periods of |sum_k conj(p[k]) x[q W5 + n + k]|^2 / sum_k |x[...]|^2 (0 where the energy is 0).  Every lag is
    one row of a freshly built array, summed the same way whatever the other rows hold."""
    x = np.asarray(x).astype(np.complex128)
    W5 = 75 * N
    lags = np.asarray(lags, dtype=np.int64)
    C = np.zeros((len(reps), len(lags)))
    idx = lags[:, None] + np.arange(N)[None, :]
    for q in range(P):
        win = x[q * W5 + idx]
        e = np.sum(win.real ** 2 + win.imag ** 2, axis=1)
        for r, p in enumerate(reps):
            a = np.sum(win * np.conj(np.asarray(p).astype(np.complex128))[None, :], axis=1)
            C[r] += np.where(e > 0.0, (a.real ** 2 + a.imag ** 2) / np.where(e > 0.0, e, 1.0), 0.0)
    return C


def corr_full(x, reps, N, P):
    """the same for all 75 N lags, through FFTs (float64: equal to corr_direct to ~1e-12 relative)"""
    x = np.asarray(x).astype(np.complex128)
    W5 = 75 * N
    L = 1 << int(math.ceil(math.log2(W5 + N)))
    C = np.zeros((len(reps), W5))
    F = [np.conj(np.fft.fft(np.asarray(p).astype(np.complex128), L)) for p in reps]
    for q in range(P):
        seg = x[q * W5:q * W5 + W5 + N - 1]
        X = np.fft.fft(seg, L)
        pw = np.concatenate([[0.0], np.cumsum(seg.real ** 2 + seg.imag ** 2)])
        e = pw[N:N + W5] - pw[:W5]
        for r in range(len(reps)):
            a = np.fft.ifft(X * F[r])[:W5]
            C[r] += np.where(e > 1e-30, (a.real ** 2 + a.imag ** 2) / np.where(e > 1e-30, e, 1.0), 0.0)
    return C


def window(bn, N, W5=None):
    """the lags a cancellation at bn changes: 2 N - 1 lags from bn - (N - 1) on, modulo W5 -> dict(n_lo, n_lag, runs: consecutive runs, the one at 0 second)"""
    W5 = 75 * N if W5 is None else W5
    n_lo, n_lag = (bn - (N - 1)) % W5, 2 * N - 1
    runs = [(n_lo, n_lag)] if n_lo + n_lag <= W5 else [(n_lo, W5 - n_lo), (0, n_lag - (W5 - n_lo))]
    return dict(n_lo=n_lo, n_lag=n_lag, runs=runs)


def window_lags(bn, N, W5=None):
    W5 = 75 * N if W5 is None else W5
    w = window(bn, N, W5)
    return (w["n_lo"] + np.arange(w["n_lag"])) % W5


# ---------------- cancellation ----------------
def cancel(x, p, N, P, bn, with_bound=False):
    """residual and the gains a_j of the P + 1 occurrences at bn + j 75 N: a_j = sum_k conj(p[k]) x[.. + k], x[.. + k] -= a_j p[k].
    with_bound: also what a float32 evaluation may be off by, per component - (N + 3) 2^-24 times the sum of magnitudes of the dot product (any order of
    summation of N products), carried through the product a_j p[k] (two products, one sum) and the subtraction."""
    x = np.asarray(x).astype(np.complex128)
    p = np.asarray(p).astype(np.complex128)
    W5 = 75 * N
    res = x.copy()
    a = np.zeros(P + 1, dtype=np.complex128)
    ba = np.zeros((P + 1, 2))
    br = np.zeros((len(x), 2))
    g = (N + 3) * U
    for j in range(P + 1):
        lo = bn + j * W5
        v = x[lo:lo + N]
        a[j] = np.sum(v * np.conj(p))
        ba[j, 0] = g * float(np.sum(np.abs(v.real * p.real) + np.abs(v.imag * p.imag)))
        ba[j, 1] = g * float(np.sum(np.abs(v.imag * p.real) + np.abs(v.real * p.imag)))
        res[lo:lo + N] = v - a[j] * p
        m_re = np.abs(a[j].real * p.real) + np.abs(a[j].imag * p.imag)
        m_im = np.abs(a[j].real * p.imag) + np.abs(a[j].imag * p.real)
        e_re = ba[j, 0] * np.abs(p.real) + ba[j, 1] * np.abs(p.imag)
        e_im = ba[j, 0] * np.abs(p.imag) + ba[j, 1] * np.abs(p.real)
        br[lo:lo + N, 0] = e_re + 3.0 * U * (m_re + e_re) + U * (np.abs(v.real) + m_re + e_re)
        br[lo:lo + N, 1] = e_im + 3.0 * U * (m_im + e_im) + U * (np.abs(v.imag) + m_im + e_im)
    return (res, a, br, ba) if with_bound else (res, a)


# ---------------- SSS ----------------
def cp_len(N, cp):
    return (512 if cp else 144) * N // 2048


def pss_offset(N, cp):
    """first useful sample of the PSS symbol inside subframes 0 and 5"""
    c = cp_len(N, cp)
    return 5 * (N + c) + c if cp else 160 * N // 2048 + 6 * (N + c)


def _cmul_conj(a, ea, b, eb):
    """a conj(b) with per-component error bounds ea, eb -> (value, bound): two products and a sum per component"""
    v = a * np.conj(b)
    a1, b1 = np.abs(a.real) + np.abs(a.imag), np.abs(b.real) + np.abs(b.imag)
    return v, ea * b1 + eb * a1 + 2.0 * ea * eb + 3.0 * U * (a1 + 2.0 * ea) * (b1 + 2.0 * eb)


def sss_occurrence(x, p, N, n_id_2, bn, j, cp, smooth=True):
    """one occurrence under one CP hypothesis -> dict(valid, y [2] matched-filter halves, e [2] their energies, sums [336] complex, bound [336] per component)
    - the 62-carrier DFTs of the PSS symbol and of the SSS symbol N + cp samples in front of it (twiddles exp(-2 pi i k / N) rounded to float32, as a table),
    H = Ypss conj(d); smooth: H averaged over +-2 carriers inside each half of the 62 (never across DC; shorter at the edges, divided by its true length);
    z = Ysss conj(H); the 336 sums of z times the SSS sequences"""
    W5, c = 75 * N, cp_len(N, cp)
    q0 = bn + j * W5
    if q0 < N + c:
        return dict(valid=False)
    xs = np.asarray(x)
    vp = xs[q0:q0 + N].astype(np.complex128)
    vs = xs[q0 - (N + c):q0 - c].astype(np.complex128)
    pp = np.asarray(p).astype(np.complex128)
    y = np.array([np.sum(vp[h * (N // 2):(h + 1) * (N // 2)] * np.conj(pp[h * (N // 2):(h + 1) * (N // 2)])) for h in range(2)])
    e = np.array([np.sum(np.abs(vp[h * (N // 2):(h + 1) * (N // 2)]) ** 2) for h in range(2)])
    ph = -2.0 * np.pi * np.arange(N) / N
    w = (np.cos(ph).astype(np.float32) + 1j * np.sin(ph).astype(np.float32)).astype(np.complex128)
    kb = carrier_bins(N)
    tw = w[(kb[:, None] * np.arange(N)[None, :]) % N]           # [62][N]
    g = (N + 3) * U
    Y, eY = [], []
    for v in (vp, vs):
        Y.append(tw @ v)
        m = np.abs(tw.real) @ np.abs(v.real) + np.abs(tw.imag) @ np.abs(v.imag)
        m2 = np.abs(tw.imag) @ np.abs(v.real) + np.abs(tw.real) @ np.abs(v.imag)
        eY.append(g * np.maximum(m, m2))
    d = cm.pss_sequence(n_id_2).astype(np.complex64).astype(np.complex128)
    H, eH = _cmul_conj(Y[0], eY[0], d, 0.0)
    if smooth:
        Hs, eHs = np.zeros(62, dtype=np.complex128), np.zeros(62)
        for m in range(62):
            lo_h, hi_h = (0, 30) if m < 31 else (31, 61)
            lo, hi = max(lo_h, m - 2), min(hi_h, m + 2)
            n = hi - lo + 1
            Hs[m] = np.sum(H[lo:hi + 1]) / n
            mag = float(np.sum(np.maximum(np.abs(H[lo:hi + 1].real), np.abs(H[lo:hi + 1].imag))))
            eHs[m] = (float(np.sum(eH[lo:hi + 1])) + (n + 1) * U * (mag + float(np.sum(eH[lo:hi + 1])))) / n
        H, eH = Hs, eHs
    z, ez = _cmul_conj(Y[1], eY[1], H, eH)
    t = sss_table(n_id_2)
    sums = t @ z
    zm = np.maximum(np.abs(z.real), np.abs(z.imag))
    bound = float(np.sum(ez)) + (62 + 1) * U * float(np.sum(zm + ez)) + np.zeros(336)
    return dict(valid=True, y=y, e=e, sums=sums, bound=bound)


def strongest(occ):
    """the occurrence k_sync_fin takes: largest |y0 + y1|^2 / (e0 + e1) among the valid ones, the first on a tie"""
    best, jb = -1.0, 0
    for j, o in enumerate(occ):
        if not o["valid"]:
            continue
        et = float(o["e"][0] + o["e"][1])
        c = abs(o["y"][0] + o["y"][1]) ** 2 / et if et > 0.0 else 0.0
        if c > best:
            best, jb = c, j
    return jb


def sss_accumulate(x, p, N, P, n_id_2, bn):
    """-> dict(occ [2][P + 1] of sss_occurrence, acc [2][336] accumulated powers, acc_bound): the powers of the 336 sums added over the valid occurrences; on odd
    occurrences hypothesis h counts as h ^ 1 (subframes 0 and 5 alternate)"""
    occ = [[sss_occurrence(x, p, N, n_id_2, bn, j, cp) for j in range(P + 1)] for cp in range(2)]
    acc, bound = np.zeros((2, 336)), np.zeros((2, 336))
    swap = np.arange(336) ^ 1
    for cp in range(2):
        n = 0
        for j, o in enumerate(occ[cp]):
            if not o["valid"]:
                continue
            s, b = (o["sums"][swap], o["bound"][swap]) if j & 1 else (o["sums"], o["bound"])
            pw = s.real ** 2 + s.imag ** 2
            acc[cp] += pw
            bound[cp] += 2.0 * (np.abs(s.real) + np.abs(s.imag)) * b + 2.0 * b * b + 3.0 * U * pw
            n += 1
        bound[cp] += n * U * (acc[cp] + bound[cp])
    return dict(occ=occ, acc=acc, acc_bound=bound)


def decide(rnd, peak, total, W5, acc, threshold=20.0, threshold_next=THRESHOLD_NEXT, sss_ratio_min=SSS_RATIO_MIN, shared_pss_ratio=SHARED_PSS_RATIO):
    """the rule of one round on its statistics -> dict(accept, cp, best, second, runner_up, shared, p2avg, sss_ratio)
    cp: the hypothesis with the larger best power (normal on a tie); best: first maximum; second: second largest power; runner_up: the largest power among the
    hypotheses of ANOTHER N_id_1 than best's (best ^ 1 is the same cell seen half a frame off); round 0 accepts on p2avg >= threshold, later rounds on
    p2avg >= threshold_next and best / second >= sss_ratio_min; shared: runner-up power >= shared_pss_ratio x best (shared_pss_ratio < 0: never)"""
    acc = np.asarray(acc, dtype=np.float64)
    mean = total / W5
    p2avg = peak / mean if mean > 0 else 0.0
    cp = 1 if acc[1].max() > acc[0].max() else 0
    a = acc[cp]
    best = int(np.argmax(a))
    rest = a.copy()
    rest[best] = -1.0
    second = int(np.argmax(rest))
    other = np.where((np.arange(336) >> 1) != (best >> 1), a, -1.0)
    runner = int(np.argmax(other))
    ratio = a[best] / a[second] if a[second] > 0 else 0.0
    accept = p2avg >= threshold if rnd == 0 else (p2avg >= threshold_next and ratio >= sss_ratio_min)
    shared = shared_pss_ratio >= 0 and a[best] > 0 and a[runner] >= shared_pss_ratio * a[best]
    return dict(accept=bool(accept), cp=cp, best=best, second=second, runner_up=runner, shared=bool(shared), p2avg=p2avg, sss_ratio=ratio,
                best_power=a[best], second_power=a[second], runner_up_power=a[runner])


def cell_from(N, n_id_2, bn, cp, h, acc_res, with_bound=False):
    """id, timing and carrier offset of hypothesis h (at occurrence 0) by the cell search's formulas"""
    W5 = 75 * N
    occ = acc_res["occ"][cp]
    jb = strongest(occ)
    o = occ[jb]
    s = o["sums"][h ^ (jb & 1)]
    k = 15000.0 * N / (N + cp_len(N, cp))
    cfo = -math.atan2(s.imag, s.real) / (2.0 * math.pi) * k
    cfo_bound = (math.sqrt(2.0) * o["bound"][h ^ (jb & 1)] / abs(s) + 8 * U) / (2.0 * math.pi) * k + 4 * U * abs(cfo)
    coarse = math.atan2((np.conj(o["y"][0]) * o["y"][1]).imag, (np.conj(o["y"][0]) * o["y"][1]).real) / math.pi * 15000.0
    off = pss_offset(N, cp)
    sf0 = 5 if h & 1 else 0
    sf_start, sf_idx = (bn - off, sf0) if bn >= off else (bn + W5 - off, (sf0 + 5) % 10)
    out = dict(cell_id=3 * (h >> 1) + n_id_2, n_id_2=n_id_2, n_id_1=h >> 1, cp=cp, pss_pos=bn, sf_start=sf_start, sf_idx=sf_idx, cfo_hz=cfo, cfo_coarse_hz=coarse)
    if with_bound:
        out["cfo_bound"] = cfo_bound
    return out


def search_all(x, nof_prb, P=8, threshold=20.0, threshold_next=THRESHOLD_NEXT, sss_ratio_min=SSS_RATIO_MIN, shared_pss_ratio=SHARED_PSS_RATIO, max_cells=MAX_CELLS,
               with_corr=False):
    """the successive search -> list of dict(cell fields, round, shared_pss, sss_ratio, rel_power_db, p2avg)[, the correlation of each round]
    Round 0 decides as the one-cell search does: first maximum of the correlation, peak / mean of its root against threshold, SSS at the strongest occurrence
    with the channel taken carrier by carrier.  Every round also forms the accumulated decision (sss_ratio, the shared-PSS runner-up); rounds >= 1 take all
    their fields from it."""
    N = SYMBOL[nof_prb]
    W5 = 75 * N
    r = np.asarray(x)[:(P + 1) * W5 + N].astype(np.complex128)
    reps = [replica(n2, N) for n2 in range(3)]
    C = corr_full(r, reps, N, P)
    cells, corrs, pow0 = [], [], None
    rnd = 0
    while len(cells) < max_cells:
        corrs.append(C.copy())
        root = int(np.argmax(C.max(axis=1)))          # first maximum in (root, lag) order
        bn = int(np.argmax(C[root]))
        peak, total = float(C[root, bn]), float(C[root].sum())
        A = sss_accumulate(r, reps[root], N, P, root, bn)
        d = decide(rnd, peak, total, W5, A["acc"], threshold, threshold_next, sss_ratio_min, shared_pss_ratio)
        if not d["accept"]:
            break
        if rnd == 0:
            best = None
            for cp in range(2):                       # the one-cell search: one occurrence, unsmoothed channel, the larger best metric decides the CP
                jb = strongest(A["occ"][cp])
                o = sss_occurrence(r, reps[root], N, root, bn, jb, cp, smooth=False)
                pw = np.abs(o["sums"]) ** 2
                h = int(np.argmax(pw))
                if best is None or pw[h] > best[0]:
                    best = (pw[h], cp, h ^ (jb & 1), o["sums"][h])
            c = cell_from(N, root, bn, best[1], best[2], A)
            c["cfo_hz"] = -math.atan2(best[3].imag, best[3].real) / (2.0 * math.pi) * 15000.0 * N / (N + cp_len(N, best[1]))
        else:
            c = cell_from(N, root, bn, d["cp"], d["best"], A)
            if any(k["cell_id"] == c["cell_id"] for k in cells):
                break                                 # what a cancellation left of a cell is not a new cell
        r, a = cancel(r, replica(root, N, c["cfo_hz"]), N, P, bn)
        pw = float(np.mean(np.abs(a) ** 2))
        pow0 = pw if pow0 is None else pow0
        c.update(round=rnd, shared_pss=0, sss_ratio=d["sss_ratio"], p2avg=d["p2avg"], rel_power_db=10.0 * math.log10(pw / pow0))
        cells.append(c)
        if d["shared"] and len(cells) < max_cells:
            g = cell_from(N, root, bn, d["cp"], d["runner_up"], A)
            if not any(k["cell_id"] == g["cell_id"] for k in cells):
                g.update(round=rnd, shared_pss=1, sss_ratio=d["sss_ratio"], p2avg=d["p2avg"],
                         rel_power_db=c["rel_power_db"] + 10.0 * math.log10(d["runner_up_power"] / d["best_power"]))
                cells.append(g)
        if len(cells) >= max_cells:
            break
        lags = window_lags(bn, N)
        C[:, lags] = corr_direct(r, reps, N, P, lags)
        rnd += 1
    return (cells, corrs) if with_corr else cells

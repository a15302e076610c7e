"""float64 statement of the cell search over all receive antennas (lsn_cell_search_ant, k_pss_corr_ant), written from the definition:

    C[r][n] = sum_{q < P} sum_{a < A} |<p_r, x_a[q W5 + n ...]>|^2 / E_a(q, n)        (a term whose energy is 0 is skipped)

the peak, mean and p2avg of C by the one-cell search's rule (first maximum in (root, lag) order, mean of the winning root), the SSS per antenna at the common lag
(one occurrence each: the strongest whose SSS symbol lies in the buffer; channel carrier by carrier), M[h] = sum_a |hyp_a[h_a]|^2 with every antenna voting in the
parity of the first occurrence, the CP with the larger best M, the carrier offsets from the sums over the antennas.  Also the float32 bound per correlation value
the GPU test holds the kernel to.  Shares no code with the library; sequences and the per-occurrence SSS sums come from multicell_model / clock_model (themselves
restatements)."""
import math

import numpy as np

import multicell_model as MM

U = MM.U
SYMBOL = MM.SYMBOL


def _fft_len(n):
    return 1 << int(math.ceil(math.log2(n)))


def _xcorr(seg, taps, L, W5):
    """sum_k taps[k] seg[n + k] for n < W5 (taps are NOT conjugated here)"""
    return np.fft.ifft(np.fft.fft(seg, L) * np.conj(np.fft.fft(np.conj(taps), L)))[:W5]


def corr_terms(x, reps, N, P, mags=True):
    """one antenna -> per period q: (a [R][W5] complex matched-filter outputs, e [W5] window energies, m [R][W5][2] sums of magnitudes of the products that
    make the real and the imaginary part).  FFTs in float64: equal to the direct sums to ~1e-12 relative."""
    x = np.asarray(x).astype(np.complex128)
    W5 = 75 * N
    L = _fft_len(W5 + N)
    out = []
    for q in range(P):
        seg = x[q * W5:q * W5 + W5 + N - 1]
        pw = np.concatenate([[0.0], np.cumsum(seg.real ** 2 + seg.imag ** 2)])
        e = pw[N:N + W5] - pw[:W5]
        a = np.zeros((len(reps), W5), dtype=np.complex128)
        m = np.zeros((len(reps), W5, 2))
        ar_, ai_ = np.abs(seg.real), np.abs(seg.imag)
        for r, p in enumerate(reps):
            p = np.asarray(p).astype(np.complex128)
            a[r] = _xcorr(seg, np.conj(p), L, W5)
            if not mags:
                continue
            pr, pi = np.abs(p.real), np.abs(p.imag)
            m[r, :, 0] = (_xcorr(ar_, pr, L, W5) + _xcorr(ai_, pi, L, W5)).real      # re = sum v.r p.r + v.i p.i
            m[r, :, 1] = (_xcorr(ai_, pr, L, W5) + _xcorr(ar_, pi, L, W5)).real      # im = sum v.i p.r - v.r p.i
        out.append((a, e, m))
    return out


def correlation(x, reps, N, P, with_bound=False):
    """x [A][n] -> C [R][W5] (float64)[, bound [R][W5]: what a float32 evaluation with one rounding per operation may be off by, in any order of summation.
    A dot product of N products: (N + 3) 2^-24 times the sum of the magnitudes of its terms, per component and for the energy; through the square
    (2 |a| da + da^2 per component, three roundings), the quotient ((d pw + t d e) / (e - d e), one rounding) and the A P additions.]  Per antenna too: the list
    own [A] of that antenna's own C."""
    x = np.asarray(x)
    A, W5 = x.shape[0], 75 * N
    g = (N + 3) * U
    C = np.zeros((len(reps), W5))
    B = np.zeros((len(reps), W5))
    own = []
    for ant in range(A):
        Ca = np.zeros((len(reps), W5))
        for a, e, m in corr_terms(x[ant], reps, N, P, mags=with_bound):
            ok = e > 1e-30
            es = np.where(ok, e, 1.0)
            pw = a.real ** 2 + a.imag ** 2
            t = np.where(ok[None, :], pw / es[None, :], 0.0)
            Ca += t
            if with_bound:
                da_r, da_i = g * m[:, :, 0], g * m[:, :, 1]
                dpw = 2.0 * np.abs(a.real) * da_r + 2.0 * np.abs(a.imag) * da_i + da_r ** 2 + da_i ** 2
                dpw = dpw + 3.0 * U * (pw + dpw)
                de = g * es
                dt = (dpw + t * de[None, :]) / (es - de)[None, :]
                dt = dt + U * (t + dt)
                B += np.where(ok[None, :], dt, 0.0)
        own.append(Ca)
        C += Ca
    if with_bound:
        B = B + A * P * U * (C + B) + 1e-9 * C     # the additions; the last term covers the model's own FFTs
        return C, B, own
    return C, own


def _angle_cfo(s, N, cp):
    return -math.atan2(s.imag, s.real) / (2.0 * math.pi) * 15000.0 * N / (N + MM.cp_len(N, cp))


def search(x, nof_prb, P=2, threshold=20.0, force_n_id_2=-1, with_corr=False):
    """x [A][n] complex -> dict(found, cell_id, n_id_2, n_id_1, cp, pss_pos, sf_start, sf_idx, pss_peak, pss_p2avg, sss_metric, sss_second, cfo_hz, cfo_bound,
    cfo_coarse_hz, per_ant: [dict(pss_peak, sss_metric, sss_second, cfo_hz, n_id_1, occurrence)])[, C [3][W5] (rows of roots not searched are 0)]"""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None, :]
    A, N = x.shape[0], SYMBOL[nof_prb]
    W5 = 75 * N
    x = x[:, :(P + 1) * W5 + N]
    roots = [force_n_id_2] if force_n_id_2 >= 0 else [0, 1, 2]
    reps = [MM.replica(r, N) for r in roots]
    C, own = correlation(x, reps, N, P)
    i = int(np.argmax(C.reshape(-1)))                    # the first maximum in (root, lag) order
    ri, bn = divmod(i, W5)
    root = roots[ri]
    peak, mean = float(C[ri, bn]), float(np.mean(C[ri]))
    p2avg = peak / mean if mean > 0 else 0.0
    swap = np.arange(336) ^ 1
    best = None
    for cp in range(2):
        votes, bounds, ys, js, raws = [], [], [], [], []
        for ant in range(A):
            occ = [MM.sss_occurrence(x[ant], reps[ri], N, root, bn, j, cp, smooth=False) for j in range(P + 1)]
            jb = MM.strongest(occ)
            o = occ[jb]
            raws.append(o["sums"])
            votes.append(o["sums"][swap] if jb & 1 else o["sums"])
            bounds.append(o["bound"][swap] if jb & 1 else o["bound"])
            ys.append(o["y"])
            js.append(jb)
        M = sum(np.abs(v) ** 2 for v in votes)
        h = int(np.argmax(M))
        if best is None or M[h] > best["M"][best["h"]]:   # normal CP on a tie
            best = dict(cp=cp, h=h, M=M, votes=votes, bounds=bounds, ys=ys, js=js, raws=raws)
    cp, h, M = best["cp"], best["h"], best["M"]
    rest = M.copy()
    rest[h] = -1.0
    s = sum(v[h] for v in best["votes"])
    k = 15000.0 * N / (N + MM.cp_len(N, cp))
    cfo = _angle_cfo(s, N, cp)
    sb = sum(float(b[h]) for b in best["bounds"]) + A * U * sum(abs(v[h].real) + abs(v[h].imag) for v in best["votes"])
    cfo_bound = (math.sqrt(2.0) * sb / abs(s) + 8 * U) / (2.0 * math.pi) * k + 4 * U * abs(cfo) if abs(s) > 0 else float("inf")
    yy = sum(np.conj(y[0]) * y[1] for y in best["ys"])
    off = MM.pss_offset(N, cp)
    sf0 = 5 if h & 1 else 0
    sf_start, sf_idx = (bn - off, sf0) if bn >= off else (bn + W5 - off, (sf0 + 5) % 10)
    per = []
    for ant in range(A):
        pw = np.abs(best["raws"][ant]) ** 2
        ah = int(np.argmax(pw))
        r2 = pw.copy()
        r2[ah] = -1.0
        per.append(dict(pss_peak=float(own[ant][ri, bn]), sss_metric=float(pw[ah]), sss_second=float(r2.max()), cfo_hz=_angle_cfo(best["raws"][ant][ah], N, cp),
                        n_id_1=ah >> 1, vote=(ah ^ (best["js"][ant] & 1)), occurrence=best["js"][ant]))
    out = dict(found=bool(p2avg >= threshold), cell_id=3 * (h >> 1) + root, n_id_2=root, n_id_1=h >> 1, cp=cp, pss_pos=bn, sf_start=sf_start, sf_idx=sf_idx,
               pss_peak=peak, pss_p2avg=p2avg, sss_metric=float(M[h]), sss_second=float(rest.max()), cfo_hz=cfo, cfo_bound=cfo_bound,
               cfo_coarse_hz=math.atan2(yy.imag, yy.real) / math.pi * 15000.0, per_ant=per)
    if not with_corr:
        return out
    full = np.zeros((3, W5))
    for ri_, r in enumerate(roots):
        full[r] = C[ri_]
    return out, full

"""Float64 statement of the per-grant uplink arrival-time measurement (k_pusch_toa, k_ul_fft_win of ltesniffer_amd/csrc/kernels/ul_timing.hip; test
infrastructure only): the estimator, the window decision, the re-cut under the zero rule, the float32 error bound of the estimator, and the list of
(cell, grant, arrival) points the GPU tests run (tests/test_gpu_ul_timing.py).  tests/test_ul_timing_model.py checks all of it on the CPU oracle.

Geometry.  A subframe that arrives `a` samples EARLY is `iq[a:]` followed by zeros (early()); a negative a is a late arrival.  The common SC-FDMA
window then starts a samples into every symbol: the carriers get the phase ramp exp(+2 pi j k a / N) and the last a samples of the window belong to the
next symbol's cyclic prefix.

Estimator.  ls_s[n] = y_s[n] conj(r_s[n]) on the reference-signal symbol of slot s (r from tests/spec_uplink.py: written from 36.211 5.5, not from the
product's tables), z = sum_s sum_{n = 0}^{M - 2} ls_s[n + 1] conj(ls_s[n]), tau = arg(z) N / 2 pi in samples, positive = early.  Lever arm: one carrier
spacing; the 2 (M - 1) products add coherently, so the slope is averaged over the whole allocation.  Unambiguous for |tau| < N / 2.

Decision (decide()).  shift = rint(tau) (ties to even), clamped to [-late_max, +max_advance], 0 when |shift| < min_shift.  Defaults: min_shift =
max(1, N / 128), max_advance = N / 4, late_max = 144 N / 2048.

Re-cut (recut()).  Symbol l is read at pos_l - shift; a sample index in front of the subframe or behind its end reads as zero - which is the common
window on the buffer s[i] = buf[i - shift] (zero outside).  The oracle run on s is the truth of the second pass.

Float32 bound (f32_bound()).  What the kernel computes differs from this model by
  * the reference sequence: base value and cyclic-shift phasor each rounded to float32 (u = 2^-24 each) and one complex product (3 u): 5 u;
  * ls = y conj(r): 3 u more, 8 u per estimate; a product of two estimates 8 + 8 + 3 = 19 u, taken as 20 u relative to its modulus;
  * the sum: thread t adds ceil(2 M / 256) terms one after the other, then 8 tree levels: (ceil(2 M / 256) + 8) u relative to S = sum |product|;
  so |dz| <= g u S with g = 28 + ceil(2 M / 256), and the angle moves by at most 1.01 g u S / |z| (asin x <= 1.01 x for x < 0.1, asserted);
  * atan2f: 6 ulp (the OpenCL bound for atan2, which the device library meets) of the angle: 6 u |phi|;
  * times N, divided by float32(2 pi): two roundings and the constant's own: 3 u |tau|.
  bound = N / 2 pi (1.01 g u S / |z| + 6 u |phi|) + 3 u |tau|."""
import functools

import numpy as np

import spec_uplink as SU
from lsn_testlib import pusch_hop_slot1

U32 = 2.0 ** -24
FLAG_CLAMPED, FLAG_BELOW = 1, 2


def early(iq, a):
    """the subframe as it lies in the common window when it arrives a samples early (a < 0: late): zeros where nothing of it is"""
    iq = np.asarray(iq)
    z = np.zeros(abs(a), dtype=iq.dtype)
    return np.concatenate([iq[a:], z]) if a >= 0 else np.concatenate([z, iq[:a]])


def recut(buf, shift):
    """the zero rule: s[i] = buf[i - shift], zero outside the subframe; the common window on s is the window moved `shift` samples earlier on buf"""
    return early(buf, -shift)


def thresholds(N, min_shift=0, max_advance=0):
    return (min_shift or max(1, N // 128), max_advance or N // 4, 144 * N // 2048)


def decide(tau, N, min_shift=0, max_advance=0):
    """-> (shift, flags); tau as the float32 the kernel holds"""
    mn, mx, late = thresholds(N, min_shift, max_advance)
    s, f = int(np.rint(np.float32(tau))), 0
    if s > mx:
        s, f = mx, f | FLAG_CLAMPED
    if s < -late:
        s, f = -late, f | FLAG_CLAMPED
    if abs(s) < mn:
        s, f = 0, f | FLAG_BELOW
    return s, f


def ls_estimates(cell, sf_idx, rg, grid):
    """grid: complex [14 * nre] (rows = symbols); rg: receiver_grant dict -> ls[2, M] complex128"""
    nre, nsl, M = 12 * cell["nof_prb"], 6 if cell["cp"] else 7, 12 * rg["L_prb"]
    g = np.asarray(grid, dtype=np.complex128).reshape(-1, nre)
    out = np.zeros((2, M), dtype=np.complex128)
    for s in range(2):
        k0 = 12 * (rg["n_prb2"] if (s and rg.get("hop")) else rg["n_prb"])
        y = g[nsl - 4 + nsl * s, k0:k0 + M]
        out[s] = y * np.conj(SU.dmrs(cell, 2 * sf_idx + s, rg["n_dmrs"], M))
    return out


def toa(cell, sf_idx, rg, grid):
    """-> dict(tau, phi, z, S, E, conf, bound): the estimator in float64 and the float32 bound of the module docstring for this input"""
    N = SU.FFT[cell["nof_prb"]]
    ls = ls_estimates(cell, sf_idx, rg, grid)
    p = ls[:, 1:] * np.conj(ls[:, :-1])
    z, S, E = p.sum(), np.abs(p).sum(), (np.abs(ls) ** 2).sum()
    phi = float(np.angle(z)) if z != 0 else 0.0
    tau = phi * N / (2 * np.pi)
    return dict(tau=tau, phi=phi, z=z, S=S, E=E, conf=abs(z) / E if E > 0 else 0.0, bound=f32_bound(N, ls.shape[1], S, abs(z), phi))


def f32_bound(N, M, S, absz, phi):
    g = 28 + -(-2 * M // 256)
    x = g * U32 * S / absz if absz > 0 else np.inf
    assert x < 0.1, ("the estimate is too weak for the small-angle step of the bound", x)
    return N / (2 * np.pi) * (1.01 * x + 6 * U32 * abs(phi)) + 3 * U32 * abs(phi) * N / (2 * np.pi)


# ---------------------------------------------------------------------------------------------------------------------------- the points of the GPU tests
# cells of the timing tests: one per (bandwidth, cyclic prefix)
def cell_of(prb, cp):
    return dict(nof_prb=prb, cell_id={6: 301, 25: 196, 100: 77}[prb] + cp, cp=cp, cyclic_shift=(3 + cp) % 8, delta_ss=5 * cp, group_hopping=0, sequence_hopping=0,
                hopping_offset=2 if prb == 25 else 0)


# (a): name -> (prb, first PRB, L, mcs, hopping bits or None).  The arrival estimate of a short grant far outside the prefix depends on the data of the
# neighbouring symbols (the ISI is part of the least-squares estimates), so a point is one realisation: TOA_SEED names, per (grant, cyclic prefix), the first
# seed (counted from 0) at which the float64 tau of EVERY arrival of toa_arrivals() - and of the re-cut points (b) that use the grant - lies at least 0.25 away
# from a half-integer, so that a float32 atan2f cannot change the shift.  test_ul_timing_model.py asserts that property for every point.
TOA_GRANTS = {"6prb_L1": (6, 4, 1, 4, None), "6prb_L3": (6, 2, 3, 9, None), "25prb_L3": (25, 10, 3, 9, None), "25prb_L24": (25, 1, 24, 16, None),
              "25prb_hop": (25, 3, 3, 9, 0), "100prb_L96": (100, 2, 96, 16, None)}
TOA_SEED = {("6prb_L1", 0): 1, ("6prb_L1", 1): 10, ("6prb_L3", 0): 2, ("6prb_L3", 1): 1, ("25prb_L3", 0): 0, ("25prb_L3", 1): 14, ("25prb_L24", 0): 0,
            ("25prb_L24", 1): 0, ("25prb_hop", 0): 2, ("25prb_hop", 1): 14, ("100prb_L96", 0): 0, ("100prb_L96", 1): 0}
TOA_SF = 3
LATE = -3
HALF_MARGIN = 0.25


def half_distance(tau):
    """distance of tau from the nearest half-integer"""
    return abs((tau - 0.5) - round(tau - 0.5))


def toa_arrivals(N):
    return (0, 1, 17, N // 16, N // 4, LATE)


@functools.lru_cache(maxsize=None)
def one_grant(prb, cp, n, L, mcs, hop=None, seed=0, sf=TOA_SF):
    """one noise-free grant of unit gain -> (cell, sf_idx, iq[15 N], truth)"""
    cell = cell_of(prb, cp)
    qm, tbs = SU.tbs_of(mcs, L)
    g = dict(rnti=0x1234 + 7 * seed + prb, n_prb=n, L_prb=L, mod=qm, tbs=tbs, rv=0, n_dmrs=(seed + 2) % 8, gain_db=0.0, phase=0.7 + seed, nof_ack=0, ri_bits=0, cqi_bits=0)
    if hop is not None:
        g.update(hop=1, n_prb2=pusch_hop_slot1(prb, cell["hopping_offset"], hop, n))
    iq, truths = SU.subframe(cell, sf, [g], seed=4000 + 10 * seed + cp)
    return cell, sf, iq, truths[0]


def toa_case(name, cp):
    prb, n, L, mcs, hop = TOA_GRANTS[name]
    return one_grant(prb, cp, n, L, mcs, hop, TOA_SEED[(name, cp)])


# (b): re-cut inside the first prefix (normal cyclic prefix): grant of (a) -> arrivals
RECUT_EXACT = {"25prb_L24": (0, 1, 17, 40), "100prb_L96": (160,)}
# (c): the rows of the issue's table: (prb, first PRB, L, mcs, arrival, decodes in the common window, seed).  At a = N / 4 on three PRB the ISI moves the estimate
# by several samples from one realisation to the next (seeds 0 .. 7 at 100 PRB, a = 512: tau = 494.5, 529.0, 505.2, 503.0, 510.9, 512.3, 513.6, 519.8; at 6 PRB,
# a = 32: 29.9, 30.3, 33.8, 32.7, 32.2, 30.7, 31.9, 30.7 - every one of them decodes after the re-cut).  The seed of a row is the first (from 0) at which the
# row's listed verdict in the common window, round(tau) within 1 % of a plus one sample, the same for the residual, and HALF_MARGIN all hold in float64.
TABLE = [
    (25, 9, 6, 16, 32, True, 2), (25, 9, 6, 16, 64, False, 1),
    (25, 10, 3, 9, 64, True, 2), (25, 10, 3, 9, 128, False, 0),
    (100, 2, 96, 16, 128, False, 0),
    (100, 40, 3, 9, 512, False, 4),
    (6, 2, 3, 9, 32, False, 4),
]


def table_case(row):
    prb, n, L, mcs, a, _, seed = row
    return one_grant(prb, 0, n, L, mcs, None, seed)


def arrival_tolerance(a):
    """the issue's accuracy statement: 1 % of the arrival plus one sample"""
    return 0.01 * abs(a) + 1.0


TWO_UE_SEED = 2


@functools.lru_cache(maxsize=None)
def two_ues(seed=TWO_UE_SEED, prb=25):
    """(d): two QPSK UEs (MCS 10) of equal power on one subframe, two PRB between them, arrivals 0 and N / 8 -> (cell, sf_idx, iq, truths, arrivals)"""
    cell = cell_of(prb, 0)
    N = SU.FFT[prb]
    out, truths = np.zeros(15 * N, dtype=np.complex128), []
    arr = (0, N // 8)
    for k, (n, L, a) in enumerate(((3, 4, arr[0]), (9, 6, arr[1]))):
        qm, tbs = SU.tbs_of(10, L)
        g = dict(rnti=0x2001 + k + 16 * seed, n_prb=n, L_prb=L, mod=qm, tbs=tbs, rv=0, n_dmrs=(3 + k + seed) % 8, gain_db=0.0, phase=1.1 * k, nof_ack=0, ri_bits=0, cqi_bits=0)
        iq, t = SU.subframe(cell, TOA_SF, [g], seed=4100 + k + 10 * seed)
        out += early(iq.astype(np.complex128), a)
        truths.append(t[0])
    return cell, TOA_SF, out.astype(np.complex64), truths, arr

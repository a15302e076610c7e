// lsn_dsp.h - device helpers that more than one kernel file uses: complex products, the symbol transform of the downlink (k_ofdm, stage_a.hip)
// and the uplink (k_ul_fft, stage_ul.hip), the soft demodulator of PDSCH (stage_c.hip) and PUSCH (stage_ul.hip).
// Float arithmetic is written one rounding per operation (compiled with -ffp-contract=off): the operation order of every expression here is part of the
// parity contract with the tests' CPU oracle.  (stage_sync.hip keeps its own products: its sums keep one component only.)
#pragma once
#include "lsn_dev.h"
#include "lsn_fft_map.h"

__device__ __forceinline__ cf32 cmul(cf32 a, cf32 b) { cf32 c; c.r = a.r * b.r - a.i * b.i; c.i = a.r * b.i + a.i * b.r; return c; }
__device__ __forceinline__ cf32 cmulconj(cf32 a, cf32 b) { cf32 c; c.r = a.r * b.r + a.i * b.i; c.i = a.i * b.r - a.r * b.i; return c; }
__device__ __forceinline__ float cabs2(cf32 a) { return a.r * a.r + a.i * a.i; }

// ------------------------------------------------------------------------------------------------ symbol transform
// The oracle's radix-2 decimation in time, run in passes of R stages on 2^R registers; lsn_fft_map.h says which thread holds which elements and where they
// lie in LDS.  R stages on one group: e[j] = v[base + j 2^S], low = base mod 2^S; tw[(1 << q) - 1 + m] is the twiddle of stage S + q at offset low + m 2^S
template <int R, int S, int LG>
__device__ __forceinline__ void fft_twiddles(cf32* tw, const cf32* __restrict__ W, int low)
{
#pragma unroll
  for (int q = 0; q < R; q++)
#pragma unroll
    for (int m = 0; m < (1 << q); m++) tw[(1 << q) - 1 + m] = W[lsn_fft_twiddle(low + (m << S), S + q, LG)];
}
template <int R>
__device__ __forceinline__ void fft_butterflies(cf32* e, const cf32* tw)
{
#pragma unroll
  for (int q = 0; q < R; q++) {
#pragma unroll
    for (int j = 0; j < (1 << R); j++) {
      if (j & (1 << q)) continue;
      cf32 v = cmul(e[j + (1 << q)], tw[(1 << q) - 1 + (j & ((1 << q) - 1))]);
      cf32 uu = e[j];
      e[j].r = uu.r + v.r; e[j].i = uu.i + v.i;
      e[j + (1 << q)].r = uu.r - v.r; e[j + (1 << q)].i = uu.i - v.i;
    }
  }
}
// one pass from LDS to LDS
template <int R, int S, int LG, int NB>
__device__ __forceinline__ void fft_pass(cf32* a, const cf32* __restrict__ W, int tid)
{
  constexpr int G = 1 << R, NG = NB << (LG - R);
#pragma unroll
  for (int u = 0; u < (NG + LSN_FFT_THREADS - 1) / LSN_FFT_THREADS; u++) {
    const int gg = tid + LSN_FFT_THREADS * u;
    if (gg < NG) {
      const int r = NB == 1 ? 0 : gg >> (LG - R), g = gg & ((1 << (LG - R)) - 1), base = lsn_fft_base(g, S, R);
      const int at = lsn_fft_store(r, base, LG);
      cf32 e[G], tw[G - 1];
#pragma unroll
      for (int j = 0; j < G; j++) e[j] = a[at ^ lsn_fft_slot(j << S)];
      fft_twiddles<R, S, LG>(tw, W, base & ((1 << S) - 1));
      fft_butterflies<R>(e, tw);
#pragma unroll
      for (int j = 0; j < G; j++) a[at ^ lsn_fft_slot(j << S)] = e[j];
    }
  }
}
// the last pass of a power-of-two size: from LDS to the carriers of the grid row; pw (LDS, may lie over a; null: not wanted) receives |X|^2 per carrier
template <int R, int LG>
__device__ __forceinline__ void fft_last_pass(cf32* a, const cf32* __restrict__ W, cf32* __restrict__ out, float* pw, int nre, int dc, int tid)
{
  constexpr int G = 1 << R, S = LG - R, NG = 1 << S, U = (NG + LSN_FFT_THREADS - 1) / LSN_FFT_THREADS;
  cf32 e[U][G], tw[U][G - 1];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int g = tid + LSN_FFT_THREADS * u;
    if (g < NG) {
      const int at = lsn_fft_store(0, g, LG);
#pragma unroll
      for (int j = 0; j < G; j++) e[u][j] = a[at ^ lsn_fft_slot(j << S)];
      fft_twiddles<R, S, LG>(tw[u], W, g);
    }
  }
  if (pw) __syncthreads();  // every read of a is done before pw goes over it
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int g = tid + LSN_FFT_THREADS * u;
    if (g < NG) {
      fft_butterflies<R>(e[u], tw[u]);
#pragma unroll
      for (int j = 0; j < G; j++) {
        const int k = lsn_fft_carrier(g + (j << S), 1 << LG, nre, dc);
        if (k >= 0) {
          out[k] = e[u][j];
          if (pw) pw[k] = e[u][j].r * e[u][j].r + e[u][j].i * e[u][j].i;
        }
      }
    }
  }
}
// pass 0 from the time samples, then every later pass
template <int LG, int NB, typename Load>
__device__ __forceinline__ void fft_run(const LsnCellDev& c, cf32* a, Load load, cf32* __restrict__ out, float* pw, int dc, int tid)
{
  constexpr int M = 1 << LG, N = NB * M;
  const cf32* __restrict__ W = c.twiddle;
  const int nre = (int)c.nre;
  if (tid < N / 8) {
    cf32 x[8], e[8], tw[7];
#pragma unroll
    for (int jj = 0; jj < 8; jj++) x[jj] = load(lsn_fft_first_sample(tid, jj, N));
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = x[lsn_fft_brev3(j)];
    fft_twiddles<3, 0, LG>(tw, W, 0);
    fft_butterflies<3>(e, tw);
    int r, g;
    lsn_fft_first_group(tid, NB, LG, &r, &g);
    const int at = lsn_fft_store(r, 8 * g, LG);
#pragma unroll
    for (int j = 0; j < 8; j++) a[at ^ lsn_fft_slot(j)] = e[j];
  }
  __syncthreads();
  constexpr int R1 = LG >= 6 ? 3 : LG - 3, S2 = 3 + R1, R2 = LG - S2 >= 3 ? 3 : LG - S2, S3 = S2 + R2, R3 = LG - S3;  // lsn_fft_radix: 7 <= LG <= 11
  static_assert(LG >= 7 && LG <= 11 && R2 >= 1 && R3 >= 0 && R3 <= 2, "pass plan");
  static_assert(R1 == 3 && (R3 == 0 || R2 == 3), "pass plan");
  fft_pass<R1, 3, LG, NB>(a, W, tid);
  __syncthreads();
  if constexpr (R3 > 0) {
    fft_pass<R2, S2, LG, NB>(a, W, tid);
    __syncthreads();
  }
  constexpr int RL = R3 > 0 ? R3 : R2, SL = LG - RL;
  if constexpr (NB == 1) {
    fft_last_pass<RL, LG>(a, W, out, pw, nre, dc, tid);
  } else {
    // N = 3 M: X[k] = (F_0[k % M] + F_1[k % M] T[k]) + F_2[k % M] T[2 k mod N] for the carriers that are kept
    fft_pass<RL, SL, LG, NB>(a, W, tid);
    __syncthreads();
    const cf32* __restrict__ T = c.twiddle3;
    float p[6];  // nre <= 1320
#pragma unroll
    for (int it = 0; it < 6; it++) {
      const int k = tid + LSN_FFT_THREADS * it;
      if (k < nre) {
        const int bin = lsn_fft_carrier_bin(k, N, nre, dc), kq = bin & (M - 1);
        int b2 = 2 * bin;
        b2 = b2 >= N ? b2 - N : b2;
        const cf32 f0 = a[lsn_fft_store(0, kq, LG)];
        const cf32 t1 = cmul(a[lsn_fft_store(1, kq, LG)], T[bin]), t2 = cmul(a[lsn_fft_store(2, kq, LG)], T[b2]);
        const float sr = f0.r + t1.r, si = f0.i + t1.i;
        cf32 X;
        X.r = sr + t2.r;
        X.i = si + t2.i;
        out[k] = X;
        p[it] = X.r * X.r + X.i * X.i;
      }
    }
    if (pw) {
      __syncthreads();
#pragma unroll
      for (int it = 0; it < 6; it++) {
        const int k = tid + LSN_FFT_THREADS * it;
        if (k < nre) pw[k] = p[it];
      }
    }
  }
}
// The N-point transform of one OFDM / SC-FDMA symbol by a workgroup of 256 threads: a is LDS, N cf32; load(n) gives time sample n (with whatever
// rotation the caller applies), out receives the c.nre occupied carriers.  dc = 1: the carrier map skips the DC bin (downlink), 0: it does not (uplink).
// pw: null, or nre floats of LDS (a itself will do) that receive |X[k]|^2 of the carriers; the caller synchronises before it reads them.
// The twiddles come from c.twiddle (L1 / L2): pass 0 reads them through the scalar cache, a later pass reads at most seven entries per thread.
template <typename Load>
__device__ __forceinline__ void lsn_symbol_fft(const LsnCellDev& c, cf32* a, Load load, cf32* out, float* pw, int dc, int tid)
{
  if (c.twiddle3) {
    switch ((int)c.lgN) {
      case 7: fft_run<7, 3>(c, a, load, out, pw, dc, tid); break;
      case 8: fft_run<8, 3>(c, a, load, out, pw, dc, tid); break;
      default: fft_run<9, 3>(c, a, load, out, pw, dc, tid); break;
    }
    return;
  }
  switch ((int)c.lgN) {
    case 7: fft_run<7, 1>(c, a, load, out, pw, dc, tid); break;
    case 8: fft_run<8, 1>(c, a, load, out, pw, dc, tid); break;
    case 9: fft_run<9, 1>(c, a, load, out, pw, dc, tid); break;
    case 10: fft_run<10, 1>(c, a, load, out, pw, dc, tid); break;
    default: fft_run<11, 1>(c, a, load, out, pw, dc, tid); break;
  }
}

// ------------------------------------------------------------------------------------------------ soft demodulation
// max-log soft bits of one QPSK / 16QAM / 64QAM / 256QAM symbol (36.211 7.1), L[0 .. Qm)
__device__ __forceinline__ void lsn_demod_llr(int Qm, float I, float Q, float* L)
{
  float aI = fabsf(I), aQ = fabsf(Q);
  L[0] = -I; L[1] = -Q;
  if (Qm == 4) {
    const float a = 0.31622776601683794f;
    L[2] = aI - 2.0f * a; L[3] = aQ - 2.0f * a;
  } else if (Qm == 6) {
    const float a = 0.15430334996209191f;
    float tI = aI - 4.0f * a, tQ = aQ - 4.0f * a;
    L[2] = tI; L[3] = tQ; L[4] = fabsf(tI) - 2.0f * a; L[5] = fabsf(tQ) - 2.0f * a;
  } else if (Qm == 8) {
    const float a = 0.07669649888473704f;
    float tI = aI - 8.0f * a, tQ = aQ - 8.0f * a;
    float uI = fabsf(tI) - 4.0f * a, uQ = fabsf(tQ) - 4.0f * a;
    L[2] = tI; L[3] = tQ; L[4] = uI; L[5] = uQ; L[6] = fabsf(uI) - 2.0f * a; L[7] = fabsf(uQ) - 2.0f * a;
  }
}

// lsn_dsp.h - device helpers that more than one kernel file uses: complex products, the LDS-staged symbol transform of the downlink (k_ofdm, stage_a.hip)
// and the uplink (k_ul_fft, stage_ul.hip), the soft demodulator of PDSCH (stage_c.hip) and PUSCH (stage_ul.hip).
// Float arithmetic is written one rounding per operation (compiled with -ffp-contract=off): the operation order of every expression here is part of the
// parity contract with the tests' CPU oracle.  (stage_sync.hip keeps its own products: its sums keep one component only.)
#pragma once
#include "lsn_dev.h"

__device__ __forceinline__ cf32 cmul(cf32 a, cf32 b) { cf32 c; c.r = a.r * b.r - a.i * b.i; c.i = a.r * b.i + a.i * b.r; return c; }
__device__ __forceinline__ cf32 cmulconj(cf32 a, cf32 b) { cf32 c; c.r = a.r * b.r + a.i * b.i; c.i = a.i * b.r - a.r * b.i; return c; }
__device__ __forceinline__ float cabs2(cf32 a) { return a.r * a.r + a.i * a.i; }

// ------------------------------------------------------------------------------------------------ symbol transform
// one radix-2^R decimation-in-time pass over the N bit-reversed points in a (LDS), 256 threads; w = exp(-2 pi i k / 2^lgN), s = stages already done
template <int R>
__device__ __forceinline__ void fft_pass(cf32* a, const cf32* w, int s, int N, int lgN, int tid)
{
  constexpr int G = 1 << R;
  const int h = 1 << s;
#pragma unroll
  for (int u = 0; u < (8 >> R); u++) {
    int g = tid * (8 >> R) + u;
    if (g >= (N >> R)) break;
    int low = g & (h - 1), high = g >> s, base = (high << (s + R)) | low;
    cf32 e[G];
#pragma unroll
    for (int j = 0; j < G; j++) e[j] = a[base + j * h];
#pragma unroll
    for (int q = 0; q < R; q++) {
#pragma unroll
      for (int j = 0; j < G; j++) {
        if (j & (1 << q)) continue;
        int pos = low + (j & ((1 << q) - 1)) * h;
        cf32 v = cmul(e[j + (1 << q)], w[pos << (lgN - (s + q + 1))]);
        cf32 uu = e[j];
        e[j].r = uu.r + v.r; e[j].i = uu.i + v.i;
        e[j + (1 << q)].r = uu.r - v.r; e[j + (1 << q)].i = uu.i - v.i;
      }
    }
#pragma unroll
    for (int j = 0; j < G; j++) a[base + j * h] = e[j];
  }
}
// all passes of NB transforms of M = 2^lgN points that lie side by side in a: lgN = 9 is three radix-8 passes per block, 8 = 8, 8, 4 and 7 = 8, 8, 2
template <int NB>
__device__ __forceinline__ void fft_passes(cf32* a, const cf32* w, int M, int lgN, int tid)
{
  for (int s = 0; s < lgN;) {
    const int left = lgN - s;
    if (left >= 3) { for (int r = 0; r < NB; r++) fft_pass<3>(a + r * M, w, s, M, lgN, tid); s += 3; }
    else if (left == 2) { for (int r = 0; r < NB; r++) fft_pass<2>(a + r * M, w, s, M, lgN, tid); s += 2; }
    else { for (int r = 0; r < NB; r++) fft_pass<1>(a + r * M, w, s, M, lgN, tid); s += 1; }
    __syncthreads();
  }
}
// The N-point transform of one OFDM / SC-FDMA symbol by a workgroup of 256 threads: a [N] and w [N / 2] are LDS, load(n) gives time sample n (with
// whatever rotation the caller applies), out receives the c.nre occupied carriers.  dc = 1: the carrier map skips the DC bin (downlink), 0: it does not
// (uplink).  Twiddle staging, bit-reversed scatter, radix-8/4/2 passes, the radix-3 combination where N = 3 x 2^k, carrier extraction.
template <typename Load>
__device__ __forceinline__ void lsn_symbol_fft(const LsnCellDev& c, cf32* a, cf32* w, Load load, cf32* out, int dc, int tid)
{
  const int N = (int)c.N, lgN = (int)c.lgN, nre = (int)c.nre;
  if (c.twiddle3) {
    // N = 3 M with M = 128 / 256 / 512 (384, 768, 1536): x_r[m] = x[3 m + r] -> three M-point transforms side by side in LDS, then
    // X[k] = (F_0[k % M] + F_1[k % M] T[k]) + F_2[k % M] T[2 k mod N] for the carriers that are kept
    const int M = (int)c.nsub;
    for (int n = tid; n < M / 2; n += 256) w[n] = c.twiddle[n];
    for (int n = tid; n < N; n += 256) {
      const cf32 x = load(n);
      const int m = n / 3, r = n - 3 * m;
      a[r * M + (int)(__brev((unsigned)m) >> (32 - lgN))] = x;
    }
    __syncthreads();
    fft_passes<3>(a, w, M, lgN, tid);
    const cf32* __restrict__ T = c.twiddle3;
    for (int k = tid; k < nre; k += 256) {
      const int bin = (k < nre / 2) ? (N - nre / 2 + k) : (k - nre / 2 + dc), kq = bin & (M - 1);
      int b2 = 2 * bin;
      b2 = b2 >= N ? b2 - N : b2;
      const cf32 t1 = cmul(a[M + kq], T[bin]), t2 = cmul(a[2 * M + kq], T[b2]);
      const float sr = a[kq].r + t1.r, si = a[kq].i + t1.i;
      cf32 X;
      X.r = sr + t2.r;
      X.i = si + t2.i;
      out[k] = X;
    }
    return;
  }
  for (int n = tid; n < N / 2; n += 256) w[n] = c.twiddle[n];
  for (int n = tid; n < N; n += 256) a[__brev((unsigned)n) >> (32 - lgN)] = load(n);
  __syncthreads();
  fft_passes<1>(a, w, N, lgN, tid);
  for (int k = tid; k < nre; k += 256) out[k] = a[(k < nre / 2) ? (N - nre / 2 + k) : (k - nre / 2 + dc)];
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

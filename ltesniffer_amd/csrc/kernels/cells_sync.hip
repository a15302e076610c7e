// cells_sync.hip - the kernels of the successive cell search (gfx950; host: lsn_sync_all.cc): every cell of a carrier, not only the strongest.
//
// k_pss_cancel     one workgroup per PSS occurrence j of an accepted cell: a_j = sum_k conj(p[k]) r[bn + j W5 + k] (p: the unit-energy replica rotated by the cell's
//                  carrier offset), then r[...] -= a_j p[k].  Lane t adds k = t, t + 256, ... in index order, the 256 partial sums meet in a fixed LDS tree.
// k_pss_corr_win   k_pss_corr's expression for C[root][n] (stage_sync.hip: same staging, same order of operations, so the same bits) on a run of consecutive
//                  lags [n_lo, n_lo + n_lag) only - after a cancellation the lags with |n - bn| < N (mod W5) are the ones whose samples changed.
// k_sync_fin_acc   grid (CP hypothesis, occurrence): k_sync_fin's quantities for EVERY occurrence whose SSS symbol is inside the buffer - the matched filter
//                  halves, the two 62-carrier DFTs, the channel from the PSS averaged over +-2 carriers inside each half of the band, the 336 coherent sums.
// k_sync_fin_pow   grid (CP hypothesis): the powers of those sums added over the occurrences in index order; on odd occurrences hypothesis h counts as h ^ 1
//                  (subframe 0 and 5 alternate).
// Every sum runs in a fixed order (compiled with -ffp-contract=off): results depend on nothing but the input.
#include "lsn_dev.h"

#define CELLS_TILE 256
#define CELLS_MAX_OCC 17

__global__ __launch_bounds__(CELLS_TILE) void k_pss_cancel(cf32* __restrict__ r, const cf32* __restrict__ p /* [N] */, uint32_t N, uint32_t W5, uint32_t bn,
                                                           float* __restrict__ a_out /* [gridDim.x][2] */)
{
  __shared__ float sr[CELLS_TILE], si[CELLS_TILE];
  const uint32_t t = threadIdx.x, j = blockIdx.x;
  cf32* rj = r + (size_t)j * W5 + bn;  // bn < W5, j <= P: the last sample is below (P + 1) W5 + N
  float ar = 0.0f, ai = 0.0f;
  for (uint32_t k = t; k < N; k += CELLS_TILE) {
    const cf32 v = rj[k], a = p[k];
    ar = ar + (v.r * a.r + v.i * a.i);
    ai = ai + (v.i * a.r - v.r * a.i);
  }
  sr[t] = ar; si[t] = ai;
  __syncthreads();
  for (uint32_t h = CELLS_TILE / 2; h > 0; h >>= 1) {
    if (t < h) {
      sr[t] = sr[t] + sr[t + h];
      si[t] = si[t] + si[t + h];
    }
    __syncthreads();
  }
  ar = sr[0]; ai = si[0];
  for (uint32_t k = t; k < N; k += CELLS_TILE) {
    cf32 v = rj[k];
    const cf32 a = p[k];
    v.r = v.r - (ar * a.r - ai * a.i);
    v.i = v.i - (ar * a.i + ai * a.r);
    rj[k] = v;
  }
  if (t == 0) {
    a_out[2 * j] = ar;
    a_out[2 * j + 1] = ai;
  }
}

__global__ __launch_bounds__(CELLS_TILE) void k_pss_corr_win(const cf32* __restrict__ x, const cf32* __restrict__ p /* [nroots][N] */, uint32_t N, uint32_t W5,
                                                             uint32_t P, uint32_t nroots, uint32_t n_lo, uint32_t n_lag, float* __restrict__ C /* [nroots][W5] */)
{
  __shared__ cf32 xs[CELLS_TILE + 2048];
  const cf32* __restrict__ ps = p;  // uniform index: scalar loads
  const uint32_t t = threadIdx.x, n0 = n_lo + blockIdx.x * CELLS_TILE, n = n0 + t;
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  for (uint32_t q = 0; q < P; q++) {
    __syncthreads();
    const cf32* xq = x + (size_t)q * W5 + n0;
    for (uint32_t i = t; i < CELLS_TILE + N; i += CELLS_TILE) xs[i] = xq[i];  // n0 < n_lo + n_lag <= W5 and 256 < W5: below (P + 1) W5 + N
    __syncthreads();
    float ar0 = 0.0f, ai0 = 0.0f, ar1 = 0.0f, ai1 = 0.0f, ar2 = 0.0f, ai2 = 0.0f, e = 0.0f;
    if (nroots == 3) {
      for (uint32_t k = 0; k < N; k++) {
        const cf32 v = xs[t + k];
        const cf32 a = ps[k], b = ps[N + k], d = ps[2 * N + k];
        e = e + (v.r * v.r + v.i * v.i);
        ar0 = ar0 + (v.r * a.r + v.i * a.i);
        ai0 = ai0 + (v.i * a.r - v.r * a.i);
        ar1 = ar1 + (v.r * b.r + v.i * b.i);
        ai1 = ai1 + (v.i * b.r - v.r * b.i);
        ar2 = ar2 + (v.r * d.r + v.i * d.i);
        ai2 = ai2 + (v.i * d.r - v.r * d.i);
      }
    } else {
      for (uint32_t k = 0; k < N; k++) {
        const cf32 v = xs[t + k];
        const cf32 a = ps[k];
        e = e + (v.r * v.r + v.i * v.i);
        ar0 = ar0 + (v.r * a.r + v.i * a.i);
        ai0 = ai0 + (v.i * a.r - v.r * a.i);
      }
    }
    if (e > 0.0f) {
      c0 = c0 + (ar0 * ar0 + ai0 * ai0) / e;
      c1 = c1 + (ar1 * ar1 + ai1 * ai1) / e;
      c2 = c2 + (ar2 * ar2 + ai2 * ai2) / e;
    }
  }
  if (n < n_lo + n_lag) {
    C[n] = c0;
    if (nroots == 3) {
      C[W5 + n] = c1;
      C[2 * (size_t)W5 + n] = c2;
    }
  }
}

struct LsnSyncOcc {     // one (CP hypothesis, occurrence)
  uint32_t valid;       // the SSS symbol of this occurrence lies inside the buffer
  float y[2][3];        // matched filter halves of the PSS symbol: re, im, energy
  float hyp[336][2];    // coherent SSS sums per hypothesis h = 2 N_id_1 + (subframe 5)
};

__global__ __launch_bounds__(512) void k_sync_fin_acc(const cf32* __restrict__ x, const cf32* __restrict__ p /* [N] replica of the round's root */,
                                                      const cf32* __restrict__ w /* [N] exp(-2 pi i k / N) */, const cf32* __restrict__ d /* [62] PSS sequence */,
                                                      const int8_t* __restrict__ sss /* [336][62] */, uint32_t N, uint32_t W5, uint32_t bn, uint32_t cp0,
                                                      uint32_t cp1, LsnSyncOcc* __restrict__ out /* [2][gridDim.y] */)
{
  __shared__ cf32 Y[2][62];
  __shared__ cf32 H[62];
  __shared__ cf32 z[62];
  const uint32_t t = threadIdx.x, j = blockIdx.y, cp = blockIdx.x ? cp1 : cp0;
  LsnSyncOcc* o = out + (size_t)blockIdx.x * gridDim.y + j;
  const size_t q0 = (size_t)j * W5 + bn;
  if (q0 < (size_t)N + cp) {  // the SSS symbol starts in front of the buffer (uniform: the whole workgroup leaves)
    if (t == 0) o->valid = 0;
    return;
  }
  if (t == 0) o->valid = 1;
  if (t >= 128 && t < 130) {  // a wavefront of its own, beside the DFT lanes
    const uint32_t h = t - 128;
    const cf32* xj = x + q0;
    float ar = 0.0f, ai = 0.0f, e = 0.0f;
    for (uint32_t k = h * (N / 2); k < (h + 1) * (N / 2); k++) {
      const cf32 v = xj[k], a = p[k];
      ar = ar + (v.r * a.r + v.i * a.i);
      ai = ai + (v.i * a.r - v.r * a.i);
      e = e + (v.r * v.r + v.i * v.i);
    }
    o->y[h][0] = ar; o->y[h][1] = ai; o->y[h][2] = e;
  }
  if (t < 124) {
    const uint32_t s = t / 62, m = t % 62;
    const uint32_t kb = m < 31 ? N - 31 + m : m - 30;
    const cf32* xx = s ? x + q0 - (N + cp) : x + q0;
    float ar = 0.0f, ai = 0.0f;
    uint32_t idx = 0;  // (kb * n) mod N
    for (uint32_t n = 0; n < N; n++) {
      const cf32 v = xx[n], ww = w[idx];
      ar = ar + (v.r * ww.r - v.i * ww.i);
      ai = ai + (v.r * ww.i + v.i * ww.r);
      idx += kb;
      idx = idx >= N ? idx - N : idx;
    }
    Y[s][m].r = ar;
    Y[s][m].i = ai;
  }
  __syncthreads();
  if (t < 62) {
    const cf32 yp = Y[0][t], dd = d[t];
    H[t].r = yp.r * dd.r + yp.i * dd.i;  // H = Ypss conj(d)
    H[t].i = yp.i * dd.r - yp.r * dd.i;
  }
  __syncthreads();
  if (t < 62) {
    // mean of H over +-2 carriers, inside the half of the band the carrier is in (DC lies between carriers 30 and 31); shorter at the edges
    const uint32_t lo_h = t < 31 ? 0u : 31u, hi_h = t < 31 ? 30u : 61u;
    const uint32_t lo = t >= lo_h + 2 ? t - 2 : lo_h, hi = t + 2 <= hi_h ? t + 2 : hi_h;
    float hr = 0.0f, hi_ = 0.0f;
    for (uint32_t m = lo; m <= hi; m++) {
      hr = hr + H[m].r;
      hi_ = hi_ + H[m].i;
    }
    const float cnt = (float)(hi - lo + 1);
    hr = hr / cnt;
    hi_ = hi_ / cnt;
    const cf32 ys = Y[1][t];
    z[t].r = ys.r * hr + ys.i * hi_;  // z = Ysss conj(H)
    z[t].i = ys.i * hr - ys.r * hi_;
  }
  __syncthreads();
  if (t < 336) {
    const int8_t* sq = sss + (size_t)t * 62;
    float ar = 0.0f, ai = 0.0f;
    for (int m = 0; m < 62; m++) {
      const float sg = (float)sq[m];
      ar = ar + z[m].r * sg;
      ai = ai + z[m].i * sg;
    }
    o->hyp[t][0] = ar;
    o->hyp[t][1] = ai;
  }
}

__global__ __launch_bounds__(384) void k_sync_fin_pow(const LsnSyncOcc* __restrict__ occ /* [2][nocc] */, uint32_t nocc, float* __restrict__ acc /* [2][336] */)
{
  const uint32_t t = threadIdx.x, c = blockIdx.x;
  if (t >= 336) return;
  float s = 0.0f;
  for (uint32_t j = 0; j < nocc; j++) {
    const LsnSyncOcc* o = occ + (size_t)c * nocc + j;
    if (!o->valid) continue;
    const uint32_t h = t ^ (j & 1u);
    const float ar = o->hyp[h][0], ai = o->hyp[h][1];
    s = s + (ar * ar + ai * ai);
  }
  acc[c * 336 + t] = s;
}

// r: (P + 1) W5 + N samples, written; a_out: [P + 1][2]
void lsn_launch_pss_cancel(cf32* r, const cf32* p, uint32_t N, uint32_t W5, uint32_t P, uint32_t bn, float* a_out, hipStream_t s)
{
  if (N < 1 || N > 2048 || P + 1 > CELLS_MAX_OCC || bn >= W5 || W5 < N) throw std::runtime_error("k_pss_cancel: bad geometry");
  LSN_LAUNCH(k_pss_cancel, dim3(P + 1), dim3(CELLS_TILE), 0, s, r, p, N, W5, bn, a_out);
}
// one run of consecutive lags [n_lo, n_lo + n_lag), n_lo + n_lag <= W5 (a window that wraps is two runs: lsn_sync_all.h)
void lsn_launch_pss_corr_win(const cf32* x, const cf32* p, uint32_t N, uint32_t W5, uint32_t P, uint32_t nroots, uint32_t n_lo, uint32_t n_lag, float* C, hipStream_t s)
{
  if (!n_lag) return;
  if (N < 1 || N > 2048 || W5 <= CELLS_TILE || n_lo >= W5 || n_lag > W5 - n_lo || !P || (nroots != 1 && nroots != 3)) throw std::runtime_error("k_pss_corr_win: bad geometry");
  LSN_LAUNCH(k_pss_corr_win, dim3((n_lag + CELLS_TILE - 1) / CELLS_TILE), dim3(CELLS_TILE), 0, s, x, p, N, W5, P, nroots, n_lo, n_lag, C);
}
// occ: [2][P + 1] LsnSyncOcc, acc: [2][336]
void lsn_launch_sync_fin_acc(const cf32* x, const cf32* p, const cf32* w, const cf32* d, const int8_t* sss, uint32_t N, uint32_t W5, uint32_t P, uint32_t bn, uint32_t cp0,
                             uint32_t cp1, void* occ, float* acc, hipStream_t s)
{
  if (N < 64 || N > 2048 || P + 1 > CELLS_MAX_OCC || bn >= W5) throw std::runtime_error("k_sync_fin_acc: bad geometry");
  LSN_LAUNCH(k_sync_fin_acc, dim3(2, P + 1), dim3(512), 0, s, x, p, w, d, sss, N, W5, bn, cp0, cp1, (LsnSyncOcc*)occ);
  LSN_LAUNCH(k_sync_fin_pow, dim3(2), dim3(384), 0, s, (const LsnSyncOcc*)occ, P + 1, acc);
}

// sync_ant.hip - the PSS correlation of the cell search added over the receive antennas of a recording (gfx950).
//
// k_pss_corr_ant   k_pss_corr (stage_sync.hip) with one more loop: per lag n and root r
//                      C[r][n] = sum_{q < P} sum_{a < A} |<p_r, x_a[q W5 + n ...]>|^2 / E_a(q, n)      (a term with E_a(q, n) == 0 is skipped)
//                  q outer, a inner, one float accumulator per root, every expression k_pss_corr's with one rounding per operation (-ffp-contract=off): with
//                  A = 1 the result has k_pss_corr's bits.  The antennas are added AFTER the matched filter and the division (non-coherent): their channels
//                  are independent, and samples added before the filter cancel a cell whose two channels are opposite.
//                  256 lags per workgroup, blockIdx.y = channel of a bank; antenna a of channel c starts at x + c x_stride + a ant_stride, so a buffer
//                  [antenna][sample] and the carrier scan's bank [antenna][hypothesis][sample] are both read in place.  The 256 + N samples of one
//                  (period, antenna) are staged one after the other in ONE LDS image (18 KB whatever A is); lane t reads xs[t + k] (consecutive 8-byte words:
//                  conflict free by the bank rule), the replica taps are wave-uniform (scalar loads).
//                  lag0 / nlag: the lags lag0 .. lag0 + nlag - 1 only, written to C[r W5 + n - lag0] (the search asks for each antenna's own value at the
//                  common peak this way: A = 1, one channel per antenna, one lag).
//                  The unroll factors are the ones the compiler chooses for k_pss_corr by itself; under two outer loops it leaves the tap loops rolled, one
//                  tap and three waited-for scalar loads per trip.  With them the tap loops are k_pss_corr's instruction for instruction.
#include "lsn_dev.h"

#define SYNC_TILE 256

__global__ __launch_bounds__(SYNC_TILE) void k_pss_corr_ant(const cf32* __restrict__ x, const cf32* __restrict__ p /* [nroots][N] */, uint32_t N, uint32_t W5, uint32_t P,
                                                            uint32_t nroots, uint32_t A, uint32_t lag0, uint32_t nlag, float* __restrict__ C /* [nroots][W5] */,
                                                            size_t x_stride, size_t ant_stride, size_t c_stride)
{
  x += (size_t)blockIdx.y * x_stride;
  C += (size_t)blockIdx.y * c_stride;
  __shared__ cf32 xs[SYNC_TILE + 2048];
  const cf32* __restrict__ ps = p;  // uniform index: scalar loads
  const uint32_t t = threadIdx.x, m0 = blockIdx.x * SYNC_TILE, n0 = lag0 + m0;
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  for (uint32_t q = 0; q < P; q++) {
    for (uint32_t a = 0; a < A; a++) {
      __syncthreads();
      const cf32* xq = x + (size_t)a * ant_stride + (size_t)q * W5 + n0;
      for (uint32_t i = t; i < SYNC_TILE + N; i += SYNC_TILE) xs[i] = xq[i];  // an antenna holds (P + 1) W5 + N samples and W5 >= 256 (launcher): in range
      __syncthreads();
      float ar0 = 0.0f, ai0 = 0.0f, ar1 = 0.0f, ai1 = 0.0f, ar2 = 0.0f, ai2 = 0.0f, e = 0.0f;
      if (nroots == 3) {
#pragma unroll 4
        for (uint32_t k = 0; k < N; k++) {
          const cf32 v = xs[t + k];
          const cf32 g = ps[k], b = ps[N + k], d = ps[2 * N + k];
          e = e + (v.r * v.r + v.i * v.i);
          ar0 = ar0 + (v.r * g.r + v.i * g.i);
          ai0 = ai0 + (v.i * g.r - v.r * g.i);
          ar1 = ar1 + (v.r * b.r + v.i * b.i);
          ai1 = ai1 + (v.i * b.r - v.r * b.i);
          ar2 = ar2 + (v.r * d.r + v.i * d.i);
          ai2 = ai2 + (v.i * d.r - v.r * d.i);
        }
      } else {
#pragma unroll 8
        for (uint32_t k = 0; k < N; k++) {
          const cf32 v = xs[t + k];
          const cf32 g = ps[k];
          e = e + (v.r * v.r + v.i * v.i);
          ar0 = ar0 + (v.r * g.r + v.i * g.i);
          ai0 = ai0 + (v.i * g.r - v.r * g.i);
        }
      }
      if (e > 0.0f) {  // power over the energy of the window, as k_pss_corr
        c0 = c0 + (ar0 * ar0 + ai0 * ai0) / e;
        c1 = c1 + (ar1 * ar1 + ai1 * ai1) / e;
        c2 = c2 + (ar2 * ar2 + ai2 * ai2) / e;
      }
    }
  }
  const uint32_t m = m0 + t;
  if (m < nlag) {
    C[m] = c0;
    if (nroots == 3) {
      C[W5 + m] = c1;
      C[2 * (size_t)W5 + m] = c2;
    }
  }
}

// nch channels of A antennas each (declared in host/lsn_sync_ant.h)
void lsn_launch_pss_corr_ant(const cf32* x, size_t x_stride, size_t ant_stride, uint32_t A, const cf32* p, uint32_t N, uint32_t W5, uint32_t P, uint32_t nroots, uint32_t lag0,
                             uint32_t nlag, float* C, size_t c_stride, uint32_t nch, hipStream_t s)
{
  if (!nch || !nlag) return;
  if (N < 1 || N > 2048 || W5 < SYNC_TILE || nch > 65535 || !A || (nroots != 1 && nroots != 3) || lag0 >= W5 || nlag > W5 - lag0)
    throw std::runtime_error("k_pss_corr_ant: bad geometry");
  LSN_LAUNCH(k_pss_corr_ant, dim3((nlag + SYNC_TILE - 1) / SYNC_TILE, nch), dim3(SYNC_TILE), 0, s, x, p, N, W5, P, nroots, A, lag0, nlag, C, x_stride, ant_stride, c_stride);
}

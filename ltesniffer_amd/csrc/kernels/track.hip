// track.hip - the timing error detector of a stream's timing loop (gfx950; host: lsn_track.cc, lsn_stream_ring.cc) and, further down, the
// search over a whole half frame that finds a lost cell again (k_pss_acquire).
//
// k_pss_timing  the matched filter of the cell's PSS replica at 13 lags l_j = (j - 6) d around the place p where the PSS symbol's useful part starts in a subframe
//               of a Phy's block buffer ([subframe][antenna][sflen] cf32):
//                 C_j = sum_a | sum_k x_a[p + l_j + k] conj r[k] |^2 / sum_a sum_k |x_a[p + l_j + k]|^2        (0 when the denominator is 0)
//               k_pss_track (stage_sync.hip) gives one lane per lag; 13 lags would idle four fifths of a wavefront and leave the N taps of a lag to one lane.  Here
//               the workgroup works on the correlation index: grid (occurrences, cells), 256 lanes, lane t takes k = t, t + 256, ... for ALL 13 lags (a replica tap is
//               loaded once and used 13 times; lane t reads xs[j d + k], consecutive 8-byte words across the wavefront: conflict free).  The N + 12 d samples of
//               one antenna (at most 2240, 17.5 KB) are staged in LDS.  The 39 partial sums of a lane (re, im, energy of 13 lags) are reduced in a FIXED tree:
//               a butterfly over the wavefront by lane exchange (xor 32, 16, ... 1: every lane ends with the same bits, additions commute), then the four
//               wavefronts' sums through LDS in the order ((w0 + w1) + (w2 + w3)).  So the 13 values are a function of the buffer's contents and of nothing else:
//               not of the launch's other occurrences or cells, not of timing.  The cells' arguments travel in the kernel argument block, as k_resample_cells'.
#include "lsn_dev.h"
#include "../host/lsn_track_launch.h"
#include <algorithm>
#include <cstring>

struct LsnTimingArgs { LsnTimingCell c[LSN_TIMING_MAX_CELLS]; };

__global__ __launch_bounds__(256) void k_pss_timing(const LsnTimingArgs P)
{
  __shared__ cf32 xs[2048 + 12 * 16];
  __shared__ float part[4][3 * LSN_TIMING_LAGS];
  const LsnTimingCell& A = P.c[blockIdx.y];
  if (blockIdx.x >= A.n_occ) return;   // the grid is as wide as the cell with the most occurrences (the whole workgroup leaves: no barrier is missed)
  const uint32_t t = threadIdx.x, N = A.N, d = A.d, len = N + 12 * d, wave = t >> 6;
  const cf32* __restrict__ rep = A.rep;
  float num = 0.0f, den = 0.0f;   // lane j < 13 of wavefront 0: the sums over the antennas of lag j
  for (uint32_t a = 0; a < A.nant; a++) {
    const cf32* __restrict__ x = A.x + ((size_t)A.sf[blockIdx.x] * A.nant + a) * A.sflen + (A.p[blockIdx.x] - 6 * d);   // the launcher keeps [p - 6 d, p + 6 d + N) inside the row
    __syncthreads();   // the antenna in front has been read
    for (uint32_t i = t; i < len; i += 256) xs[i] = x[i];
    __syncthreads();
    float ar[LSN_TIMING_LAGS], ai[LSN_TIMING_LAGS], e[LSN_TIMING_LAGS];
#pragma unroll
    for (uint32_t j = 0; j < LSN_TIMING_LAGS; j++) { ar[j] = 0.0f; ai[j] = 0.0f; e[j] = 0.0f; }
    for (uint32_t k = t; k < N; k += 256) {
      const cf32 r = rep[k];
#pragma unroll
      for (uint32_t j = 0; j < LSN_TIMING_LAGS; j++) {
        const cf32 v = xs[j * d + k];
        e[j] = e[j] + (v.r * v.r + v.i * v.i);
        ar[j] = ar[j] + (v.r * r.r + v.i * r.i);
        ai[j] = ai[j] + (v.i * r.r - v.r * r.i);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < LSN_TIMING_LAGS; j++) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        ar[j] = ar[j] + __shfl_xor(ar[j], m, 64);
        ai[j] = ai[j] + __shfl_xor(ai[j], m, 64);
        e[j] = e[j] + __shfl_xor(e[j], m, 64);
      }
      if ((t & 63) == 0) { part[wave][3 * j] = ar[j]; part[wave][3 * j + 1] = ai[j]; part[wave][3 * j + 2] = e[j]; }
    }
    __syncthreads();
    if (t < LSN_TIMING_LAGS) {
      const float sr = (part[0][3 * t] + part[1][3 * t]) + (part[2][3 * t] + part[3][3 * t]);
      const float si = (part[0][3 * t + 1] + part[1][3 * t + 1]) + (part[2][3 * t + 1] + part[3][3 * t + 1]);
      const float se = (part[0][3 * t + 2] + part[1][3 * t + 2]) + (part[2][3 * t + 2] + part[3][3 * t + 2]);
      num = num + (sr * sr + si * si);
      den = den + se;
    }
  }
  if (t < LSN_TIMING_LAGS) A.C[(size_t)blockIdx.x * LSN_TIMING_LAGS + t] = den > 0.0f ? num / den : 0.0f;
}

// k_pss_acquire  k_pss_timing's quantity at EVERY lag of a half frame, for a cell that has lost its timing (lsn_stream_reacquire): the span x
//                is 6 subframes of a search scratch in the block-buffer layout - per antenna 90 N samples contiguous in time, subframe after subframe - and
//                  C_i = sum_a | sum_k x_a[i d + k] conj r[k] |^2 / sum_a sum_k |x_a[i d + k]|^2,  i = 0 .. 75 N / d - 1       (0 when the denominator is 0)
//                Grid (lag tiles, cells), 256 lanes; a tile is LSN_ACQ_TILE = 16 consecutive lags: N + 15 d samples of one antenna (at most 2288, 17.9 KB) are
//                staged in LDS - a window that crosses a subframe boundary is gathered row by row -, 48 accumulators per lane.  The arithmetic is k_pss_timing's
//                to the letter: lane t takes k = t, t + 256, ... for all lags of its tile, the same three accumulations per (k, lag) in the same order, the same
//                tree (xor 32 .. 1, then (w0 + w1) + (w2 + w3)), the same square, antenna sum and quotient.  So C[13 N / 2 / d + j - 6] of a span is bit for bit
//                k_pss_timing's C_j on the span's first subframe (tests/test_gpu_reacq.py), and a value depends on the span's contents and on nothing else.
struct LsnAcquireArgs { LsnAcquireCell c[LSN_TIMING_MAX_CELLS]; };

__global__ __launch_bounds__(256) void k_pss_acquire(const LsnAcquireArgs P)
{
  __shared__ cf32 xs[2048 + (LSN_ACQ_TILE - 1) * 16];
  __shared__ float part[4][3 * LSN_ACQ_TILE];
  const LsnAcquireCell& A = P.c[blockIdx.y];
  if (blockIdx.x * LSN_ACQ_TILE >= A.n_lags) return;   // the grid is as wide as the cell with the most lags (the whole workgroup leaves: no barrier is missed)
  const uint32_t t = threadIdx.x, N = A.N, d = A.d, len = N + (LSN_ACQ_TILE - 1) * d, wave = t >> 6;
  const uint32_t first = blockIdx.x * LSN_ACQ_TILE * d;   // the tile's first sample, counted in time from the span's: first + len <= 76 N - d (the launcher keeps 6 sflen = 90 N)
  const cf32* __restrict__ rep = A.rep;
  float num = 0.0f, den = 0.0f;   // lane j < 16 of wavefront 0: the sums over the antennas of lag j of the tile
  for (uint32_t a = 0; a < A.nant; a++) {
    __syncthreads();   // the antenna in front has been read
    for (uint32_t i = t; i < len; i += 256) {
      const uint32_t tau = first + i, sf = tau / A.sflen;
      xs[i] = A.x[((size_t)sf * A.nant + a) * A.sflen + (tau - sf * A.sflen)];
    }
    __syncthreads();
    float ar[LSN_ACQ_TILE], ai[LSN_ACQ_TILE], e[LSN_ACQ_TILE];
#pragma unroll
    for (uint32_t j = 0; j < LSN_ACQ_TILE; j++) { ar[j] = 0.0f; ai[j] = 0.0f; e[j] = 0.0f; }
    for (uint32_t k = t; k < N; k += 256) {
      const cf32 r = rep[k];
#pragma unroll
      for (uint32_t j = 0; j < LSN_ACQ_TILE; j++) {
        const cf32 v = xs[j * d + k];
        e[j] = e[j] + (v.r * v.r + v.i * v.i);
        ar[j] = ar[j] + (v.r * r.r + v.i * r.i);
        ai[j] = ai[j] + (v.i * r.r - v.r * r.i);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < LSN_ACQ_TILE; j++) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        ar[j] = ar[j] + __shfl_xor(ar[j], m, 64);
        ai[j] = ai[j] + __shfl_xor(ai[j], m, 64);
        e[j] = e[j] + __shfl_xor(e[j], m, 64);
      }
      if ((t & 63) == 0) { part[wave][3 * j] = ar[j]; part[wave][3 * j + 1] = ai[j]; part[wave][3 * j + 2] = e[j]; }
    }
    __syncthreads();
    if (t < LSN_ACQ_TILE) {
      const float sr = (part[0][3 * t] + part[1][3 * t]) + (part[2][3 * t] + part[3][3 * t]);
      const float si = (part[0][3 * t + 1] + part[1][3 * t + 1]) + (part[2][3 * t + 1] + part[3][3 * t + 1]);
      const float se = (part[0][3 * t + 2] + part[1][3 * t + 2]) + (part[2][3 * t + 2] + part[3][3 * t + 2]);
      num = num + (sr * sr + si * si);
      den = den + se;
    }
  }
  if (t < LSN_ACQ_TILE) A.C[(size_t)blockIdx.x * LSN_ACQ_TILE + t] = den > 0.0f ? num / den : 0.0f;
}

void lsn_launch_pss_acquire(const LsnAcquireCell* cells, uint32_t n_cells, hipStream_t s)
{
  if (n_cells > LSN_TIMING_MAX_CELLS) throw std::runtime_error("k_pss_acquire: bad geometry");
  LsnAcquireArgs P;
  memset(&P, 0, sizeof(P));
  uint32_t n = 0, tiles = 0;
  for (uint32_t c = 0; c < n_cells; c++) {
    const LsnAcquireCell& k = cells[c];
    if (!k.n_lags) continue;
    if (k.N < 128 || k.N > 2048 || k.d != (k.N / 128 ? k.N / 128 : 1) || !k.nant || !k.x || !k.rep || !k.C) throw std::runtime_error("k_pss_acquire: bad geometry");
    // the last window ends at (n_lags - 1) d + N <= 76 N: inside the 6 rows of 15 N
    if (k.sflen != 15 * k.N || (uint64_t)k.n_lags * k.d != 75ull * k.N || k.n_lags % LSN_ACQ_TILE) throw std::runtime_error("k_pss_acquire: a span that is not six subframes");
    P.c[n++] = k;
    tiles = std::max(tiles, k.n_lags / LSN_ACQ_TILE);
  }
  if (!n) return;
  LSN_LAUNCH(k_pss_acquire, dim3(tiles, n), dim3(256), 0, s, P);
}

void lsn_launch_pss_timing(const LsnTimingCell* cells, uint32_t n_cells, hipStream_t s)
{
  if (n_cells > LSN_TIMING_MAX_CELLS) throw std::runtime_error("k_pss_timing: bad geometry");
  LsnTimingArgs P;
  memset(&P, 0, sizeof(P));
  uint32_t n = 0, occ = 0;
  for (uint32_t c = 0; c < n_cells; c++) {
    const LsnTimingCell& k = cells[c];
    if (!k.n_occ) continue;
    if (k.n_occ > LSN_TIMING_MAX_OCC || k.N < 128 || k.N > 2048 || k.d != (k.N / 128 ? k.N / 128 : 1) || !k.nant || !k.x || !k.rep || !k.C) throw std::runtime_error("k_pss_timing: bad geometry");
    for (uint32_t o = 0; o < k.n_occ; o++)
      if (k.p[o] < 6 * k.d || (uint64_t)k.p[o] + 6 * k.d + k.N > k.sflen) throw std::runtime_error("k_pss_timing: a window outside its subframe");
    P.c[n++] = k;
    occ = std::max(occ, k.n_occ);
  }
  if (!n) return;
  LSN_LAUNCH(k_pss_timing, dim3(occ, n), dim3(256), 0, s, P);
}

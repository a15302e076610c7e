// chanfilt.hip - the channel filter, stage 1 in front of the polyphase resampler (gfx950): a fixed-coefficient FIR of 2L + 1 taps at the recording's own rate.
// Definition: DESIGN.md section 3.1f; host side (design, refusals, spans): host/lsn_chanfilt.cc.
//
//   y1[n] = sum over k = n - L .. n + L, in that order, of g[n - k] xm[k]     one fma per product into ONE float32 accumulator per component, from 0
//   xm[n] = the recording's sample n, converted and mixed by the text k_resample stages it with (LSN_FRONT_SAMPLE, lsn_front_dev.h); 0 for n < 0
//
// One workgroup produces a tile of LSN_CF_TILE = 1024 consecutive outputs of one antenna: 256 lanes x 4 neighbouring outputs.  It stages the tile's 1024 + 2L input
// samples in LDS (converted and mixed once, zeros in front of sample 0 and outside the buffer), then every lane walks its window four staged samples - one "quad" -
// at a time: quad c of lane t is staged samples 4 (t + c) .. 4 (t + c) + 3, it meets the seven taps h[4c - 3 .. 4c + 3] and feeds sixteen products to the lane's
// four outputs.  What the polyphase tap loop cannot do and this one does:
//   - the taps are the same for every lane: h[4c .. 4c + 3] comes by scalar loads (as compiled: three s_load_dwordx2 per quad, the pairs the packed fmas
//     take; the other three of the seven taps are the previous quad's and stay in SGPRs), and a tap enters the fma as its scalar operand - no vector-cache
//     load, no VGPR;
//   - a staged sample is read from LDS once per lane and used by all four outputs: two ds_read_b128 and sixteen v_pk_fma_f32 (two fmas each, one rounding
//     each) per quad = 1/2 LDS instruction and 8 fmas per tap and lane for FOUR outputs, against 1 ds_read_b64, 1/2 global_load_dwordx4 and 2 + 1 v_fma_f32
//     per tap for ONE output in k_resample.  30 VGPRs, no scratch (gfx950, -O3).
// LDS layout: lanes are one quad = 32 bytes apart, which as one array would put every second lane of a ds_read_b128 on the same banks.  The quads are therefore
// split into two arrays - samples 0, 1 of every quad in cf_lo, samples 2, 3 in cf_hi - so that neighbouring lanes read neighbouring 16-byte words of one array:
// conflict free (the counterpart of k_chan_bank's skew, scan.hip).  2 x 512 x 16 bytes = 16 KB whatever L is.
// The products of one output run in ascending k whichever lane, tile or launch computes it, and nothing else enters it: the bits do not depend on the tiling.
// The first and the last quads of a window hold products that do not belong to every output (k outside n - L .. n + L): those quads take the guarded path - the
// guards are wave-uniform - so that no product is formed that the definition does not have (a zero tap times an infinite sample would be a NaN).
#include "lsn_front_dev.h"
#include "../host/lsn_hip.h"
#include "../host/lsn_chanfilt_launch.h"
#include <algorithm>
#include <cstring>
#include <vector>

#define LSN_CF_TILE 1024u    // outputs per workgroup (256 lanes x 4)
#define LSN_CF_QUADS 512u    // staged quads: (1024 + 2 * 512) / 4
#define LSN_CF_MAX_L 512u
#define LSN_CF_MAX_CELLS 8u

struct LsnChanFirArgs {
  const void* raw;       // input, [sample][antenna], element 0 = input sample buf_base of the recording
  int64_t buf_base;      // >= 0
  uint64_t buf_len;      // samples (per antenna) in raw
  int64_t out_first;     // n of the launch's output 0, >= 0
  uint64_t n_out;        // outputs of the launch, per antenna
  const float* taps;     // h[m] = g[m - L], m = 0 .. 2L, then zeros up to a multiple of four past 2L + 7
  uint64_t w;            // tuning word W ...
  const cf32* nco;       // ... and the NCO tables, [4096] coarse then [1024] fine; null: no mixer
  cf32* out;             // [sample][antenna]
  uint32_t L, nant;
  float scale;
  uint32_t ring_mask;    // k_chan_fir_ring: raw is a ring of ring_mask + 1 samples per antenna, sample n of the recording at slot n & ring_mask; otherwise 0, not read
};
static_assert(sizeof(LsnChanFirArgs) == 88, "the ring mask took the place of the padding: eight cells' arguments stay 704 bytes of the kernel argument block");

// RING: where sample n of the recording sits in raw - false: element n - buf_base of a linear buffer; true: slot n & ring_mask of a ring.  [buf_base, buf_base +
// buf_len) is the window of valid recording indices either way, and the window test (not the mask) is what keeps a tile from staging another lap's sample.
template <int FMT, bool RING>
__device__ __forceinline__ void chan_fir_tile(const LsnChanFirArgs& A, const bool mix, float4* cf_lo, float4* cf_hi)
{
  const uint32_t a = blockIdx.y, t = threadIdx.x, L2 = 2 * A.L;
  const uint64_t i0 = (uint64_t)blockIdx.x * LSN_CF_TILE;
  const uint32_t nt = (uint32_t)min((uint64_t)LSN_CF_TILE, A.n_out - i0);   // outputs of this tile
  const uint32_t cmax = (L2 + 3) / 4;                                       // last quad of a lane's window
  const uint32_t nstage = 4 * (256 + cmax);                                 // <= 2048: quads 0 .. 255 + cmax are read
  const uint32_t need = nt + L2;                                            // staged samples this tile's outputs read
  const int64_t n_lo = A.out_first + (int64_t)i0 - (int64_t)A.L;            // input sample staged as s = 0
  for (uint32_t s = t; s < nstage; s += 256) {
    LSN_FRONT_SAMPLE(s < need, RING ? LSN_FRONT_RING : LSN_FRONT_LINEAR, mix, A.w)
    float2* half = (float2*)((s & 2u) ? cf_hi : cf_lo);
    half[2 * (s >> 2) + (s & 1u)] = x;
  }
  __syncthreads();
  if (4 * t >= nt) return;
  const float4* h4 = (const float4*)A.taps;
  float yr[4] = {0.0f, 0.0f, 0.0f, 0.0f}, yi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float4 hp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // h[4c - 4 .. 4c - 1]
  for (uint32_t c = 0; c <= cmax; c++) {
    const float4 hc = h4[c];                         // h[4c .. 4c + 3]: the address is the same in every lane
    const float4 xa = cf_lo[t + c], xb = cf_hi[t + c];
    const float hw[7] = {hp.y, hp.z, hp.w, hc.x, hc.y, hc.z, hc.w};   // hw[j] = h[4c - 3 + j]
    const float xr[4] = {xa.x, xa.z, xb.x, xb.z}, xi[4] = {xa.y, xa.w, xb.y, xb.w};
    // staged sample 4 (t + c) + i is sample m = 4c + i - q of output q's window: tap h[m], if 0 <= m <= 2L
    if (c != 0 && 4 * c + 3 <= L2) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          yr[q] = __builtin_fmaf(hw[3 + i - q], xr[i], yr[q]);
          yi[q] = __builtin_fmaf(hw[3 + i - q], xi[i], yi[q]);
        }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int m = (int)(4 * c) + i - q;
          if (m >= 0 && m <= (int)L2) {
            yr[q] = __builtin_fmaf(hw[3 + i - q], xr[i], yr[q]);
            yi[q] = __builtin_fmaf(hw[3 + i - q], xi[i], yi[q]);
          }
        }
    }
    hp = hc;
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t o = 4 * t + (uint32_t)q;
    if (o >= nt) break;
    cf32 y; y.r = yr[q]; y.i = yi[q];
    A.out[(size_t)(i0 + o) * A.nant + a] = y;
  }
}

// grid (tiles, antennas)
template <int FMT, bool MIX>
__global__ __launch_bounds__(256) void k_chan_fir(const LsnChanFirArgs A)
{
  __shared__ float4 cf_lo[LSN_CF_QUADS], cf_hi[LSN_CF_QUADS];
  chan_fir_tile<FMT, false>(A, MIX, cf_lo, cf_hi);
}

// Several cells of one recording from ONE raw buffer in one launch (the multi-cell pass): grid (largest number of tiles of a cell, antennas, cells).
// The cells' arguments travel in the kernel argument block and are read with scalar loads, as in k_resample_cells; a cell mixes when it has NCO tables.
struct LsnChanFirCellsArgs { LsnChanFirArgs c[LSN_CF_MAX_CELLS]; };

template <int FMT>
__global__ __launch_bounds__(256) void k_chan_fir_cells(const LsnChanFirCellsArgs P)
{
  __shared__ float4 cf_lo[LSN_CF_QUADS], cf_hi[LSN_CF_QUADS];
  const LsnChanFirArgs& A = P.c[blockIdx.z];
  if ((uint64_t)blockIdx.x * LSN_CF_TILE >= A.n_out) return;
  chan_fir_tile<FMT, false>(A, A.nco != nullptr, cf_lo, cf_hi);
}

// The same launch out of a RING (lsn_stream with the filter on, lsn_channel_filter_ring): raw holds ring_mask + 1 samples per antenna and sample n of
// the recording sits at slot n & ring_mask.  Grid, argument block and early exit are k_chan_fir_cells'; a source index is below (ring_mask + 1) * nant whatever n is.
template <int FMT>
__global__ __launch_bounds__(256) void k_chan_fir_ring(const LsnChanFirCellsArgs P)
{
  __shared__ float4 cf_lo[LSN_CF_QUADS], cf_hi[LSN_CF_QUADS];
  const LsnChanFirArgs& A = P.c[blockIdx.z];
  if ((uint64_t)blockIdx.x * LSN_CF_TILE >= A.n_out) return;
  chan_fir_tile<FMT, true>(A, A.nco != nullptr, cf_lo, cf_hi);
}

void lsn::ChanFirTables::upload(const lsn::ChanFilter& f, hipStream_t s)
{
  const size_t nt = ((f.taps.size() + 7 + 3) / 4) * 4;   // the last quad's scalar load ends at h[4 ((2L + 3) / 4) + 3] <= h[2L + 6]
  std::vector<float> h(nt + (f.tune ? (4096 + 1024) * 2 : 0), 0.0f);
  std::copy(f.taps.begin(), f.taps.end(), h.begin());
  if (f.tune) lsn_nco_tables((cf32*)(h.data() + nt), (cf32*)(h.data() + nt) + 4096);
  HIP_CHECK(hipMalloc((void**)&d_taps, h.size() * sizeof(float)));
  HIP_CHECK(hipMemcpyAsync(d_taps, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));   // (h goes out of scope)
  d_nco = f.tune ? (const cf32*)(d_taps + nt) : nullptr;
}

// A cell with n_out = 0 takes no part.  One cell: k_chan_fir, the mixer a template flag; several: k_chan_fir_cells.  Out of a ring (src.ring_samples != 0, which
// lsn_ring_holds the window): k_chan_fir_ring, also for one cell
void lsn_launch_chan_fir(const LsnFrontSource& src, const LsnChanFirCell* cells, uint32_t n_cells, hipStream_t s)
{
  const uint64_t rn = src.ring_samples;
  if (n_cells > LSN_CF_MAX_CELLS || src.buf_base < 0 || !src.nant) throw std::runtime_error("k_chan_fir: bad geometry");
  if (rn && !lsn_ring_holds(rn, src.buf_len)) throw std::runtime_error("k_chan_fir_ring: bad ring");
  LsnChanFirCellsArgs P;
  memset(&P, 0, sizeof(P));
  uint32_t n = 0;
  uint64_t tiles = 0;
  for (uint32_t c = 0; c < n_cells; c++) {
    const LsnChanFirCell& k = cells[c];
    if (!k.n_out) continue;
    if (!k.L || k.L > LSN_CF_MAX_L || !k.taps || !k.out || k.out_first < 0 || k.out_first >= (int64_t)1 << 62) throw std::runtime_error("k_chan_fir: bad geometry");
    const uint64_t r = (k.n_out + LSN_CF_TILE - 1) / LSN_CF_TILE;
    if (r > 0x7FFFFFFFull) throw std::runtime_error("k_chan_fir: launch too long");
    LsnChanFirArgs& A = P.c[n++];
    A.raw = src.raw; A.buf_base = src.buf_base; A.buf_len = src.buf_len; A.out_first = k.out_first; A.n_out = k.n_out; A.taps = k.taps; A.w = k.w; A.nco = k.nco;
    A.out = k.out; A.L = k.L; A.nant = src.nant; A.scale = src.scale; A.ring_mask = rn ? (uint32_t)(rn - 1) : 0;
    tiles = std::max(tiles, r);
  }
  if (!n) return;
  if (n == 1 && !rn) {
    const LsnChanFirArgs& A = P.c[0];
    const dim3 g((uint32_t)tiles, src.nant);
    if (A.nco) LSN_LAUNCH_FMT(k_chan_fir, LSN_COMMA true, src.fmt, g, dim3(256), 0, s, A);
    else LSN_LAUNCH_FMT(k_chan_fir, LSN_COMMA false, src.fmt, g, dim3(256), 0, s, A);
    return;
  }
  const dim3 g((uint32_t)tiles, src.nant, n);
  if (!rn) LSN_LAUNCH_FMT(k_chan_fir_cells, , src.fmt, g, dim3(256), 0, s, P);
  else LSN_LAUNCH_FMT(k_chan_fir_ring, , src.fmt, g, dim3(256), 0, s, P);
}

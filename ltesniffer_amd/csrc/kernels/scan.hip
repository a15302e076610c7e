// scan.hip - the carrier scan's kernels (gfx950): a bank of narrow-band channels cut out of a wideband recording, and the peaks of their PSS correlations.
// Definition: DESIGN.md section 3.1d; host side: host/lsn_scan.cc.  The correlation itself is k_pss_corr (stage_sync.hip) with its channel dimension.
//
// k_chan_bank   grid (run of outputs, channel).  A channel is one (tuning word, antenna) pair: the scan runs H tuning words on one antenna, lsn_carrier_channel one
//               tuning word on every antenna - the same kernel, the same expressions, so a channel sample is a function of (input, configuration, hypothesis, m)
//               and of nothing else.  The arithmetic is k_resample<FMT, true>'s (64.64 positions and the integer-phase two-table NCO while staging: the one
//               text of lsn_front_dev.h; H + f dH, one fma per product in tap order); what differs is the geometry: the rate ratio goes up to 64 and the
//               taps to 768, so a run is `run` <= 256 outputs (one per lane, sized by the host so that the staged span fits in 64 KB) and the staged samples are SKEWED: sample s sits at float2 index
//               s + (s >> 5).  With the plain layout lanes are `ratio` float2 apart, ds_read_b64 banks are (byte / 4) % 64 per 32-lane half, i.e. float2 index
//               % 32: ratio 32 or 64 puts all 32 lanes of a half on one bank pair.  The skew adds the lane's multiple of 32 back in: conflict free at ratio 32,
//               2-way at 64 (table in DESIGN 3.1d).
// k_scan_peaks  grid (root, channel): maximum, first arg-max and sum (double) of one row of C - 24 bytes per (channel, root) go to the host instead of 38 KB.
#include "lsn_front_dev.h"
#include "../host/lsn_scan.h"

#define LSN_CB_LANES 256u

struct LsnChanArgs {
  const void* raw;       // input, [sample][antenna], element 0 = input sample buf_base of the recording
  int64_t buf_base;      // >= 0
  uint64_t buf_len;      // samples (per antenna) in raw
  uint64_t base_hi, base_lo;  // position of the launch's output 0
  uint64_t d_lo;         // D: fraction ...
  uint32_t d_hi;         // ... and integer part (1 .. 64)
  uint32_t taps;         // T, even
  uint32_t span;         // samples staged per run
  uint32_t run;          // outputs per workgroup, <= LSN_CB_LANES
  uint32_t nant;         // antennas interleaved in raw
  uint32_t ant0, ant_step;   // channel c reads antenna ant0 + c * ant_step ...
  uint32_t tune_step;        // ... and mixes with tunes[c * tune_step]
  uint64_t n_out;        // outputs per channel
  float scale;
  const float2* bank;    // [512][T] (H, dH)
  const uint64_t* tunes; // tuning words W
  const cf32* nco;       // [4096] coarse then [1024] fine
  cf32* out;             // output m of channel c: out[c * out_stride + m]
  size_t out_stride;
};

__device__ __forceinline__ uint32_t cb_skew(uint32_t s) { return s + (s >> 5); }

template <int FMT>
__global__ __launch_bounds__(LSN_CB_LANES) void k_chan_bank(const LsnChanArgs A)
{
  extern __shared__ float2 cb_x[];
  const uint32_t c = blockIdx.y, a = A.ant0 + c * A.ant_step, half = A.taps / 2;
  const uint64_t w = A.tunes[(size_t)c * A.tune_step];
  const uint64_t i0 = (uint64_t)blockIdx.x * A.run;
  LSN_FRONT_POSITION(i0, hi, lo)                          // of the run's first output
  const int64_t n_lo = (int64_t)hi - (int64_t)half + 1;  // input sample staged as s = 0
  for (uint32_t s = threadIdx.x; s < A.span; s += LSN_CB_LANES) {
    LSN_FRONT_SAMPLE(true, LSN_FRONT_LINEAR, true, w)
    cb_x[cb_skew(s)] = x;
  }
  __syncthreads();
  const uint64_t i = i0 + threadIdx.x;
  if (threadIdx.x >= A.run || i >= A.n_out) return;
  LSN_FRONT_POSITION(i, phi, plo)
  const uint32_t s0 = (uint32_t)((int64_t)phi - (int64_t)half + 1 - n_lo);   // first of the T staged samples of this output
  LSN_FRONT_PHASE(plo, p, f)
  if (s0 > A.span || s0 + A.taps > A.span) return;                           // cannot happen (the host sizes span); keeps the LDS reads inside
  const float4* row = (const float4*)(A.bank + (size_t)p * A.taps);
  float yr = 0.0f, yi = 0.0f;
  for (uint32_t j = 0; j < half; j++) {
    const float4 cc = row[j];
    const float c0 = __builtin_fmaf(f, cc.y, cc.x), c1 = __builtin_fmaf(f, cc.w, cc.z);
    const uint32_t s = s0 + 2 * j;
    const float2 x0 = cb_x[cb_skew(s)], x1 = cb_x[cb_skew(s + 1)];
    yr = __builtin_fmaf(c0, x0.x, yr); yi = __builtin_fmaf(c0, x0.y, yi);
    yr = __builtin_fmaf(c1, x1.x, yr); yi = __builtin_fmaf(c1, x1.y, yi);
  }
  cf32 y; y.r = yr; y.i = yi;
  A.out[(size_t)c * A.out_stride + i] = y;
}

struct LsnScanPeak {   // 24 bytes
  double sum;
  float peak;
  uint32_t lag;
  uint32_t pad[2];
};

__global__ __launch_bounds__(256) void k_scan_peaks(const float* __restrict__ C /* channel c, root r: C[c * c_stride + r * W5 ...] */, size_t c_stride, uint32_t W5,
                                                    LsnScanPeak* __restrict__ out /* [channel][gridDim.x] */)
{
  __shared__ double ssum[256];
  __shared__ float sbest[256];
  __shared__ uint32_t slag[256];
  const uint32_t t = threadIdx.x, r = blockIdx.x, c = blockIdx.y;
  const float* row = C + (size_t)c * c_stride + (size_t)r * W5;
  float best = -1.0f;
  uint32_t lag = 0;
  double sum = 0.0;
  for (uint32_t n = t; n < W5; n += 256) {
    const float v = row[n];
    sum += (double)v;
    if (v > best) { best = v; lag = n; }
  }
  ssum[t] = sum; sbest[t] = best; slag[t] = lag;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (t < h) {
      ssum[t] += ssum[t + h];
      const float b = sbest[t + h];
      const uint32_t l = slag[t + h];
      if (b > sbest[t] || (b == sbest[t] && l < slag[t])) { sbest[t] = b; slag[t] = l; }   // the FIRST maximum
    }
    __syncthreads();
  }
  if (t == 0) {
    LsnScanPeak o;
    o.sum = ssum[0]; o.peak = sbest[0]; o.lag = slag[0]; o.pad[0] = o.pad[1] = 0;
    out[(size_t)c * gridDim.x + r] = o;
  }
}

// k.nch channels of k.n_out outputs each out of src, a linear buffer (LsnChanBankLaunch: lsn_scan.h)
void lsn_launch_chan_bank(const LsnFrontSource& src, const LsnChanBankLaunch& k, hipStream_t s)
{
  if (!k.n_out || !k.nch) return;
  const size_t lds = ((size_t)k.span + ((size_t)k.span >> 5) + 1) * sizeof(float2);
  if (k.taps < 2 || (k.taps & 1) || k.span < k.taps || lds > 64 * 1024 || src.buf_base < 0 || src.ring_samples || !k.run || k.run > LSN_CB_LANES || k.nch > 65535 ||
      !src.nant || k.ant0 + (uint64_t)(k.nch - 1) * k.ant_step >= src.nant || k.out_stride < k.n_out)
    throw std::runtime_error("k_chan_bank: bad geometry");
  const uint64_t runs = (k.n_out + k.run - 1) / k.run;
  if (runs > 0x7FFFFFFFull) throw std::runtime_error("k_chan_bank: launch too long");
  LsnChanArgs A;
  A.raw = src.raw; A.buf_base = src.buf_base; A.buf_len = src.buf_len; A.base_hi = k.base_hi; A.base_lo = k.base_lo; A.d_lo = k.d_lo; A.d_hi = k.d_hi; A.taps = k.taps;
  A.span = k.span; A.run = k.run; A.nant = src.nant; A.ant0 = k.ant0; A.ant_step = k.ant_step; A.tune_step = k.tune_step; A.n_out = k.n_out; A.scale = src.scale;
  A.bank = (const float2*)k.bank; A.tunes = k.tunes; A.nco = k.nco; A.out = k.out; A.out_stride = k.out_stride;
  LSN_LAUNCH_FMT(k_chan_bank, , src.fmt, dim3((uint32_t)runs, k.nch), dim3(LSN_CB_LANES), lds, s, A);
}

// out: [nch][nroots] LsnScanPeak (24 bytes each)
void lsn_launch_scan_peaks(const float* C, size_t c_stride, uint32_t W5, uint32_t nroots, uint32_t nch, void* out, hipStream_t s)
{
  if (!nch || !nroots) return;
  if (nch > 65535 || !W5) throw std::runtime_error("k_scan_peaks: bad geometry");
  LSN_LAUNCH(k_scan_peaks, dim3(nroots, nch), dim3(256), 0, s, C, c_stride, W5, (LsnScanPeak*)out);
}

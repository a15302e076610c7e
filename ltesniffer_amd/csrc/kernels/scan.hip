// scan.hip - the carrier scan's kernels (gfx950): a bank of narrow-band channels cut out of a wideband recording, and the peaks of their PSS correlations.
// Definition: DESIGN.md section 3.1d; host side: host/lsn_scan.cc.  The correlation itself is k_pss_corr (stage_sync.hip) with its channel dimension.
//
// k_chan_bank   grid (run of outputs, channel).  A channel is one (tuning word, antenna) pair: the scan runs H tuning words on one antenna, lsn_carrier_channel one
//               tuning word on every antenna - the same kernel, the same expressions, so a channel sample is a function of (input, configuration, hypothesis, m)
//               and of nothing else.  The arithmetic is k_resample<FMT, true>'s (64.64 positions, integer-phase two-table NCO while staging, H + f dH, one fma
//               per product in tap order); what differs is the geometry: the rate ratio goes up to 64 and the taps to 768, so a run is `run` <= 256 outputs (one
//               per lane, sized by the host so that the staged span fits in 64 KB) and the staged samples are SKEWED: sample s sits at float2 index
//               s + (s >> 5).  With the plain layout lanes are `ratio` float2 apart, ds_read_b64 banks are (byte / 4) % 64 per 32-lane half, i.e. float2 index
//               % 32: ratio 32 or 64 puts all 32 lanes of a half on one bank pair.  The skew adds the lane's multiple of 32 back in: conflict free at ratio 32,
//               2-way at 64 (table in DESIGN 3.1d).
// k_scan_peaks  grid (root, channel): maximum, first arg-max and sum (double) of one row of C - 24 bytes per (channel, root) go to the host instead of 38 KB.
#include "lsn_dsp.h"

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
  // position of the run's first output: base + i0 * D
  uint64_t lo = i0 * A.d_lo, hi = __umul64hi(i0, A.d_lo) + i0 * (uint64_t)A.d_hi;
  lo += A.base_lo;
  hi += A.base_hi + (lo < A.base_lo ? 1u : 0u);
  const int64_t n_lo = (int64_t)hi - (int64_t)half + 1;  // input sample staged as s = 0
  for (uint32_t s = threadIdx.x; s < A.span; s += LSN_CB_LANES) {
    const int64_t n = n_lo + (int64_t)s, k = n - A.buf_base;
    float2 x = make_float2(0.0f, 0.0f);
    if (n >= 0 && k >= 0 && (uint64_t)k < A.buf_len) {
      const size_t src = (size_t)k * A.nant + a;
      if (FMT == 1) {
        const short2 q = ((const short2*)A.raw)[src];
        x.x = (float)q.x * A.scale; x.y = (float)q.y * A.scale;
      } else if (FMT == 2) {
        const char2 q = ((const char2*)A.raw)[src];
        x.x = (float)q.x * A.scale; x.y = (float)q.y * A.scale;
      } else {
        x = ((const float2*)A.raw)[src];
      }
      const uint64_t ph = (uint64_t)n * w;   // low 64 bits of n W
      const cf32 e = cmul(A.nco[ph >> 52], A.nco[4096u + (uint32_t)((ph >> 42) & 1023u)]);
      cf32 v; v.r = x.x; v.i = x.y;
      v = cmulconj(v, e);
      x.x = v.r; x.y = v.i;
    }
    cb_x[cb_skew(s)] = x;
  }
  __syncthreads();
  const uint64_t i = i0 + threadIdx.x;
  if (threadIdx.x >= A.run || i >= A.n_out) return;
  uint64_t plo = i * A.d_lo, phi = __umul64hi(i, A.d_lo) + i * (uint64_t)A.d_hi;
  plo += A.base_lo;
  phi += A.base_hi + (plo < A.base_lo ? 1u : 0u);
  const uint32_t s0 = (uint32_t)((int64_t)phi - (int64_t)half + 1 - n_lo);   // first of the T staged samples of this output
  const uint32_t p = (uint32_t)(plo >> 55);                                  // 9 bits of phase
  const float f = (float)(uint32_t)((plo >> 31) & 0xFFFFFFu) * 0x1p-24f;      // 24 bits inside the phase, exact
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

// nch channels of n_out outputs each from output position (base_hi, base_lo); run / span: outputs per workgroup and the samples they need (host: lsn_scan.cc).
void lsn_launch_chan_bank(const void* raw, uint32_t fmt, float scale, int64_t buf_base, uint64_t buf_len, uint64_t base_hi, uint64_t base_lo, uint32_t d_hi, uint64_t d_lo,
                          uint32_t taps, uint32_t span, uint32_t run, const float* bank, const uint64_t* tunes, uint32_t tune_step, const cf32* nco, uint32_t nant,
                          uint32_t ant0, uint32_t ant_step, uint32_t nch, cf32* out, size_t out_stride, uint64_t n_out, hipStream_t s)
{
  if (!n_out || !nch) return;
  const size_t lds = ((size_t)span + ((size_t)span >> 5) + 1) * sizeof(float2);
  if (taps < 2 || (taps & 1) || span < taps || lds > 64 * 1024 || buf_base < 0 || !run || run > LSN_CB_LANES || nch > 65535 || !nant ||
      ant0 + (uint64_t)(nch - 1) * ant_step >= nant || out_stride < n_out)
    throw std::runtime_error("k_chan_bank: bad geometry");
  const uint64_t runs = (n_out + run - 1) / run;
  if (runs > 0x7FFFFFFFull) throw std::runtime_error("k_chan_bank: launch too long");
  LsnChanArgs A;
  A.raw = raw; A.buf_base = buf_base; A.buf_len = buf_len; A.base_hi = base_hi; A.base_lo = base_lo; A.d_lo = d_lo; A.d_hi = d_hi; A.taps = taps; A.span = span;
  A.run = run; A.nant = nant; A.ant0 = ant0; A.ant_step = ant_step; A.tune_step = tune_step; A.n_out = n_out; A.scale = scale; A.bank = (const float2*)bank;
  A.tunes = tunes; A.nco = nco; A.out = out; A.out_stride = out_stride;
  const dim3 g((uint32_t)runs, nch);
  if (fmt == 1) LSN_LAUNCH((k_chan_bank<1>), g, dim3(LSN_CB_LANES), lds, s, A);
  else if (fmt == 2) LSN_LAUNCH((k_chan_bank<2>), g, dim3(LSN_CB_LANES), lds, s, A);
  else LSN_LAUNCH((k_chan_bank<0>), g, dim3(LSN_CB_LANES), lds, s, A);
}

// out: [nch][nroots] LsnScanPeak (24 bytes each)
void lsn_launch_scan_peaks(const float* C, size_t c_stride, uint32_t W5, uint32_t nroots, uint32_t nch, void* out, hipStream_t s)
{
  if (!nch || !nroots) return;
  if (nch > 65535 || !W5) throw std::runtime_error("k_scan_peaks: bad geometry");
  LSN_LAUNCH(k_scan_peaks, dim3(nroots, nch), dim3(256), 0, s, C, c_stride, W5, (LsnScanPeak*)out);
}

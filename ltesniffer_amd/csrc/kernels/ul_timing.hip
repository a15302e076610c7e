// ul_timing.hip - gfx950 kernels of the per-grant uplink arrival-time measurement (DESIGN section "Uplink arrival time"): k_pusch_toa measures how far ahead
// of the common SC-FDMA window a grant's signal arrives, from the phase slope of its reference-signal estimates, and decides on the device whether the
// grant gets a window of its own; k_ul_fft_win demodulates the grants that do once more, in a window moved to where their signal is, into a private set
// of grid rows per grant.  k_pusch_chest / k_pusch_demod (stage_ul.hip, unchanged) then run on the private rows.
// Float arithmetic: one rounding per operation, fixed summation orders, as in stage_ul.hip.
#include "lsn_dsp.h"
#include "lsn_ul_toa.h"

// fixed 256-leaf tree (the order of k_pusch_chest's and tree256_2's) on three arrays at once; result valid in thread 0
__device__ __forceinline__ void tree256_3(float* p0, float* p1, float* p2, int tid)
{
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { p0[tid] = p0[tid] + p0[tid + s]; p1[tid] = p1[tid] + p1[tid + s]; p2[tid] = p2[tid] + p2[tid + s]; }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ arrival time + decision
// one workgroup per grant: the LS estimates of both reference-signal symbols as k_pusch_chest forms them (its grid reads and sequence look-ups, a copy:
// that kernel's instruction stream is not touched), z = sum over both slots, n = 0 .. M - 2, of ls[n + 1] conj(ls[n]) (thread t adds the terms t, t + 256, ...
// of the 2 M positions in index order, then the fixed tree), tau = arg(z) N / 2 pi.  An arrival a samples ahead of the window puts the phase ramp
// exp(+2 pi j k a / N) on the carriers, so positive tau means early.
// rec: the records on the device (k_ul_fft_win reads the shift there), mirror: null or the same records in pinned host memory.
// residual_pass = 0: writes tau, shift, flags, conf of the grant's record and, when grants_out is given, a copy of the grant whose sf names the grant's
// private row set (set b for grant b).  1: the same measurement on the grid it is given, written to residual alone; no decision.
__global__ __launch_bounds__(256) void k_pusch_toa(LsnCellDev c, const LsnUlGrantDev* __restrict__ grants, const cf32* __restrict__ grid, LsnUlToaCfg cfg,
                                                   LsnUlToaDev* rec, LsnUlToaDev* mirror, LsnUlGrantDev* __restrict__ grants_out, int residual_pass)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const LsnUlGrantDev g = grants[blockIdx.x];
  const int M = 12 * (int)g.L_prb, nre = (int)c.nre, tid = threadIdx.x;
  cf32* ls = (cf32*)smem;              // [2 M]
  float* part = (float*)(ls + 2 * M);  // [3][256]
  for (int i = tid; i < 2 * M; i += 256) {
    const int s = i >= M ? 1 : 0, n = i - s * M;
    const cf32 y = grid[((size_t)g.sf * 14 + (c.nslot - 4) + c.nslot * s) * nre + 12 * (s ? g.n_prb2 : g.n_prb) + n];
    const cf32 r = cmul(c.ul_base[(s ? g.base_off1 : g.base_off) + n], c.ul_ph12[(g.ncs[s] * (uint32_t)n) % 12u]);
    ls[i] = cmulconj(y, r);
  }
  __syncthreads();
  float zr = 0.0f, zi = 0.0f, e = 0.0f;
  for (int i = tid; i < 2 * M; i += 256) {
    const int s = i >= M ? 1 : 0, n = i - s * M;
    const cf32 a = ls[i];
    e = e + (a.r * a.r + a.i * a.i);
    if (n < M - 1) {
      const cf32 p = cmulconj(ls[i + 1], a);
      zr = zr + p.r; zi = zi + p.i;
    }
  }
  part[tid] = zr; part[256 + tid] = zi; part[512 + tid] = e;
  tree256_3(part, part + 256, part + 512, tid);
  if (tid == 0) {
    const float re = part[0], im = part[256], en = part[512];
    const float tau = atan2f(im, re) * (float)c.N / 6.2831853071795864769f;
    LsnUlToaDev* o = rec + blockIdx.x;
    LsnUlToaDev* m = mirror ? mirror + blockIdx.x : o;   // pinned host memory: the record needs no copy launch of its own
    if (residual_pass) {
      o->residual = tau; m->residual = tau;
    } else {
      uint32_t flags;
      const int32_t shift = lsn_toa_decide(tau, cfg, &flags);
      const float conf = en > 0.0f ? sqrtf(re * re + im * im) / en : 0.0f;
      o->tau = tau; o->shift = shift; o->flags = flags; o->conf = conf; o->residual = 0.0f;
      m->tau = tau; m->shift = shift; m->flags = flags; m->conf = conf; m->residual = 0.0f;
    }
  }
  if (grants_out && !residual_pass) {
    // the second pass reads its grid rows at ((size_t)sf * 14 + l) * nre of the private arena
    if (tid == 0) { LsnUlGrantDev q = g; q.sf = blockIdx.x; grants_out[blockIdx.x] = q; }
  }
}

void lsn_launch_pusch_toa(const LsnCellDev& c, const LsnUlGrantDev* g, const cf32* grid, const LsnUlToaCfg& cfg, LsnUlToaDev* rec, LsnUlToaDev* mirror,
                          LsnUlGrantDev* g_out, bool residual_pass, uint32_t ngrants, hipStream_t s)
{
  LSN_LAUNCH(k_pusch_toa, dim3(ngrants), dim3(256), sizeof(cf32) * 2 * 1200 + sizeof(float) * 768, s, c, g, grid, cfg, rec, mirror, g_out, residual_pass ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------ SC-FDMA demodulation in a grant's own window
// grid (symbol, grant): k_ul_fft's body with symbol l of grant b read at pos_l - shift[b], into row set b of `priv` ([grant][14][nre]).
// The zero rule: a sample index in front of the grant's own subframe, or behind its end, reads as zero - in every subframe, so that a result never
// depends on where a chunk or a call begins.  (A shift above the first cyclic prefix therefore costs the start of symbol 0.)
// shift == 0: no transform; the workgroup copies row l of the grant's subframe from the common grid, so the second pass finds there what the one-pass
// chain reads.
__global__ __launch_bounds__(256) void k_ul_fft_win(LsnCellDev c, const cf32* __restrict__ iq, uint32_t nant, uint32_t ant, const LsnUlGrantDev* __restrict__ grants,
                                                    const LsnUlToaDev* __restrict__ rec, const cf32* __restrict__ grid, cf32* __restrict__ priv)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int N = (int)c.N, tid = threadIdx.x;
  cf32* a = (cf32*)smem;
  const int l = blockIdx.x, b = blockIdx.y;
  const int sf = (int)grants[b].sf, shift = rec[b].shift;
  const int nre = (int)c.nre;
  cf32* out = priv + ((size_t)b * 14 + l) * nre;
  if (shift == 0) {
    const cf32* src = grid + ((size_t)sf * 14 + l) * nre;
    for (int k = tid; k < nre; k += 256) out[k] = src[k];
    return;
  }
  const int cp0 = 160 * N / 2048, cp1 = 144 * N / 2048;
  const int slot = l / 7, ls = l % 7;
  const int pos = c.cp ? l * (N + N / 4) + N / 4 : slot * (cp0 + 6 * cp1 + 7 * N) + cp0 + ls * (N + cp1);
  const cf32* in = iq + ((size_t)sf * nant + ant) * c.sflen;
  const int first = pos - shift, sflen = (int)c.sflen;
  lsn_symbol_fft(c, a, [&](int n) {
    const int idx = first + n;
    cf32 x; x.r = 0.0f; x.i = 0.0f;
    if (idx >= 0 && idx < sflen) x = in[idx];
    return cmul(x, c.ul_shift[n]);
  }, out, nullptr, 0, tid);
}

void lsn_launch_ul_fft_win(const LsnCellDev& c, const cf32* iq, uint32_t nant, uint32_t ant, const LsnUlGrantDev* g, const LsnUlToaDev* rec, const cf32* grid,
                           cf32* priv, uint32_t ngrants, hipStream_t s)
{
  LSN_LAUNCH(k_ul_fft_win, dim3(c.nsym, ngrants), dim3(256), sizeof(cf32) * lsn_fft_lds_slots((int)c.N), s, c, iq, nant, ant, g, rec, grid, priv);
}

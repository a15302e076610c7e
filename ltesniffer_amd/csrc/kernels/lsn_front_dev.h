// lsn_front_dev.h - the device text that the front-end kernels share (resample.hip, chanfilt.hip, scan.hip; gfx950): the staged sample of a recording, the 64.64
// position of an output and its split into phase and fraction.  Each exists ONCE, here; file replay against stream, filtered chain against plain chain and scan
// channel against k_resample<FMT, true> compare bit for bit because the kernels expand the same expressions (DESIGN.md sections 3.1b, 3.1d, 3.1f).
//
// Macros, and not inlined __device__ functions: the compiler simplifies a function on its own before it inlines it, which reorders the instructions of the
// kernel it lands in - with the conversion and the mix as functions the SLP vectoriser pairs the NCO product differently, a few moves more per
// instantiation.  Expanded as text, every kernel of the three files is the instruction stream it was when it carried its own copy.  The macros speak the names of
// the kernel that expands them: A (its argument struct: raw, buf_base, buf_len, nant, scale, nco; base_hi, base_lo, d_lo, d_hi), FMT (its sample format), a (the
// antenna it reads) and, in the staging loop, s (the staged index) and n_lo (the recording's sample staged as s = 0).
#pragma once
#include "lsn_dsp.h"

// LSN_FRONT_SAMPLE declares n = n_lo + s (index in the RECORDING), k = n - buf_base and float2 x = sample n of antenna a, converted to float and mixed; zero in front
// of sample 0 of the recording, outside the window [buf_base, buf_base + buf_len) of indices whose samples raw holds, and where LIVE is false.
//   SRCSAMPLE  where sample n sits in A.raw: LSN_FRONT_LINEAR (element k of a linear buffer) or LSN_FRONT_RING (slot n & ring_mask of a ring of ring_mask + 1
//              samples; the window test, not the mask, keeps another lap's sample out)
//   MIXCOND    uniform over the workgroup: multiply by exp(-2 pi j Phi(n) / 2^64), Phi(n) = n W mod 2^64, through the two-table NCO of k_ofdm (A.nco: [4096] coarse
//              then [1024] fine)
#define LSN_FRONT_LINEAR k
#define LSN_FRONT_RING (n & (int64_t)A.ring_mask)
#define LSN_FRONT_SAMPLE(LIVE, SRCSAMPLE, MIXCOND, W)                                                                                                                   \
  const int64_t n = n_lo + (int64_t)s, k = n - A.buf_base;                                                                                                              \
  float2 x = make_float2(0.0f, 0.0f);                                                                                                                                   \
  if ((LIVE) && n >= 0 && k >= 0 && (uint64_t)k < A.buf_len) {                                                                                                          \
    const size_t src = (size_t)(SRCSAMPLE) * A.nant + a;                                                                                                                \
    if (FMT == 1) {                                                                                                                                                     \
      const short2 q = ((const short2*)A.raw)[src];                                                                                                                     \
      x.x = (float)q.x * A.scale; x.y = (float)q.y * A.scale;                                                                                                           \
    } else if (FMT == 2) {                                                                                                                                              \
      const char2 q = ((const char2*)A.raw)[src];                                                                                                                       \
      x.x = (float)q.x * A.scale; x.y = (float)q.y * A.scale;                                                                                                           \
    } else {                                                                                                                                                            \
      x = ((const float2*)A.raw)[src];                                                                                                                                  \
    }                                                                                                                                                                   \
    if (MIXCOND) {                                                                                                                                                      \
      const uint64_t ph = (uint64_t)n * (W);  /* low 64 bits of n W */                                                                                                  \
      const cf32 e = cmul(A.nco[ph >> 52], A.nco[4096u + (uint32_t)((ph >> 42) & 1023u)]);                                                                              \
      cf32 v; v.r = x.x; v.i = x.y;                                                                                                                                     \
      v = cmulconj(v, e);                                                                                                                                               \
      x.x = v.r; x.y = v.i;                                                                                                                                             \
    }                                                                                                                                                                   \
  }

// declares (HI, LO) = base + I * D, the 64.64 position of the launch's output I: integer part = input sample index, 64 bits of fraction
#define LSN_FRONT_POSITION(I, HI, LO)                                                                                                                                   \
  uint64_t LO = (I) * A.d_lo, HI = __umul64hi((I), A.d_lo) + (I) * (uint64_t)A.d_hi;                                                                                    \
  LO += A.base_lo;                                                                                                                                                      \
  HI += A.base_hi + (LO < A.base_lo ? 1u : 0u);

// declares P = the top 9 bits of the fraction LO (the bank's row) and F = the next 24 bits as a float in [0, 1), exact: coefficient j is H[P][j] + F * dH[P][j]
#define LSN_FRONT_PHASE(LO, P, F)                                                                                                                                       \
  const uint32_t P = (uint32_t)((LO) >> 55);                                                                                                                            \
  const float F = (float)(uint32_t)(((LO) >> 31) & 0xFFFFFFu) * 0x1p-24f;

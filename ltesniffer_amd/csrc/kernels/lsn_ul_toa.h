// lsn_ul_toa.h - the decision behind the uplink arrival-time measurement (k_pusch_toa, ul_timing.hip): which window shift a measured arrival asks
// for.  Usable on host and device: the kernel takes the decision with it, lsn_pusch_toa_decide (lsn_capi.cc) is its host mirror.  HIP-free.
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef LSN_HD
#ifdef __HIPCC__
#define LSN_HD __host__ __device__ __forceinline__
#else
#define LSN_HD static inline
#endif
#endif

#define LSN_TOA_CLAMPED 1u   // round(tau) lay outside [-late_max, +max_advance] and was moved to the bound
#define LSN_TOA_BELOW 2u     // |shift| < min_shift: the common window is kept (shift = 0)

// thresholds in samples at the cell's rate (the host resolves the defaults: min_shift N / 128, max_advance N / 4, late_max 144 N / 2048)
struct LsnUlToaCfg { int32_t min_shift, max_advance, late_max; };

// one record per grant, written by k_pusch_toa
struct LsnUlToaDev {
  float tau;        // arrival ahead of the common window in samples (positive: early), from the reference-signal phase slope
  int32_t shift;    // samples the grant's window is moved earlier (0: it stays)
  uint32_t flags;   // LSN_TOA_*
  float conf;       // |z| / sum |ls|^2: 1 for a pure delay on a flat channel, towards 0 in noise
  float residual;   // tau measured again on the re-cut symbols (mode 2 only)
  uint32_t pad[3];
};

// tau (samples) -> shift; ties of the rounding go to the even integer (rintf).  A tau that is not finite decides for no shift.
LSN_HD int32_t lsn_toa_decide(float tau, LsnUlToaCfg cfg, uint32_t* flags)
{
  uint32_t f = 0;
  if (!(tau >= -1.0e9f && tau <= 1.0e9f)) tau = 0.0f;
  int32_t s = (int32_t)rintf(tau);
  if (s > cfg.max_advance) { s = cfg.max_advance; f |= LSN_TOA_CLAMPED; }
  if (s < -cfg.late_max) { s = -cfg.late_max; f |= LSN_TOA_CLAMPED; }
  if ((s < 0 ? -s : s) < cfg.min_shift) { s = 0; f |= LSN_TOA_BELOW; }
  *flags = f;
  return s;
}

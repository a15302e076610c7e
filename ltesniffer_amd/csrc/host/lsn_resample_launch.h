// lsn_resample_launch.h - the launchers of kernels/resample.hip: the part of the resampler's host side that speaks the HIP runtime's types (lsn_resample.h, the plan,
// does not).
#pragma once
#include <hip/hip_runtime.h>
#include "lsn_resample.h"

void lsn_launch_resample(const void* raw, uint32_t fmt, float scale, int64_t buf_base, uint64_t buf_len, uint64_t base_hi, uint64_t base_lo, uint32_t d_hi,
                         uint64_t d_lo, uint32_t taps, uint32_t span, const float* bank, uint64_t w, const cf32* nco, const cf32* rot, uint32_t sflen, uint32_t sf_off,
                         uint32_t nant, cf32* out, uint64_t n_out, hipStream_t s);

// k_resample_cells: what one cell of a launch brings of its own (the launch's other arguments - raw buffer, format, scale, antennas - are the recording's)
struct LsnResampleCell {
  uint64_t base_hi, base_lo;   // position of the cell's output 0 in this launch
  uint64_t d_lo; uint32_t d_hi;
  uint32_t taps, span;
  uint32_t sflen, sf_off;
  const float* bank;
  uint64_t w; const cf32* nco; // nco null: the cell is not translated
  const cf32* rot;
  cf32* out;
  uint64_t n_out;              // 0: the cell takes no part in this launch
};
void lsn_launch_resample_cells(const void* raw, uint32_t fmt, float scale, int64_t buf_base, uint64_t buf_len, uint32_t nant, const LsnResampleCell* cells, uint32_t n_cells,
                               hipStream_t s);
// k_resample_ring: the same launch out of a device ring of ring_samples samples per antenna (a power of two), sample n of the recording at slot n & (ring_samples - 1);
// [buf_base, buf_base + buf_len) are the recording indices whose samples the ring holds, buf_len <= ring_samples
void lsn_launch_resample_ring(const void* ring, uint64_t ring_samples, uint32_t fmt, float scale, int64_t buf_base, uint64_t buf_len, uint32_t nant, const LsnResampleCell* cells,
                              uint32_t n_cells, hipStream_t s);

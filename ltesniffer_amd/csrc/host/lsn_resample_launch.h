// lsn_resample_launch.h - the part of the resampler's host side that speaks the HIP runtime's types (lsn_resample.h, the plan and the launch record, does not): the
// owner of a cell's device tables, the description of the buffer a launch reads, and the two launchers of kernels/resample.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "../../../include/ltesniffer_amd.h"
#include "lsn_resample.h"

namespace lsn {

// the bank (with the NCO tables behind it, one allocation) and the optional per-subframe rotation of one cell: allocated by upload() / rotation(), freed here
struct ResampleTables : ResampleTablePtrs {
  ResampleTables() = default;
  ResampleTables(ResampleTables&& o) noexcept : ResampleTablePtrs(o) { static_cast<ResampleTablePtrs&>(o) = ResampleTablePtrs(); }
  ~ResampleTables();
  void upload(const ResamplePlan& p, hipStream_t s);                 // device copy of p.bank and p.nco, queued on s; d_nco = null when the plan does not mix
  void rotation(float offset_freq_hz, uint32_t sflen, double fs);   // exp(-j 2 pi f n / fs), n = 0 .. sflen - 1; nothing for f = 0
};

}  // namespace lsn

// what a launch reads: [sample][antenna] in format fmt, element 0 = sample buf_base (>= 0) of the recording, buf_len samples per antenna.  ring_samples != 0: raw is
// a device ring of that many samples per antenna (a power of two), sample n of the recording at slot n & (ring_samples - 1), and [buf_base, buf_base + buf_len) are
// the recording indices whose samples the ring holds, buf_len <= ring_samples
struct LsnResampleSource {
  const void* raw; uint32_t fmt; float scale;
  int64_t buf_base; uint64_t buf_len;
  uint32_t nant;
  uint64_t ring_samples;   // 0: a linear buffer
};
void lsn_launch_resample(const LsnResampleSource& src, const LsnResampleCell& cell, hipStream_t s);                            // k_resample (a linear buffer)
void lsn_launch_resample_cells(const LsnResampleSource& src, const LsnResampleCell* cells, uint32_t n_cells, hipStream_t s);   // k_resample_cells, or k_resample_ring out of a ring

// the plan of a lsn_resample_cfg_t, validated: what lsn_resample_span and the stand-alone calls (lsn_front_launch.cc) share
int lsn_resample_plan(const lsn_resample_cfg_t* cfg, lsn::ResamplePlan& plan);

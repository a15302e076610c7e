// lsn_resample_launch.h - the part of the resampler's host side that speaks the HIP runtime's types (lsn_resample.h, the plan and the launch record, does not): the
// owner of a cell's device tables and the two launchers of kernels/resample.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "../../../include/ltesniffer_amd.h"
#include "lsn_resample.h"
#include "lsn_front_source.h"

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

// src: the buffer the launch reads (lsn_front_source.h)
// src: the recording's, its nant included; a cell with an antenna map (LsnResampleCell::map_nout) writes map_nout rows, every other cell src.nant.  When a cell of
// the launch is mapped the _map kernels run it; when none is, the kernels named here, as before the map existed
void lsn_launch_resample(const LsnFrontSource& src, const LsnResampleCell& cell, hipStream_t s);                            // k_resample (a linear buffer)
void lsn_launch_resample_cells(const LsnFrontSource& src, const LsnResampleCell* cells, uint32_t n_cells, hipStream_t s);   // k_resample_cells, or k_resample_ring out of a ring

// the plan of a lsn_resample_cfg_t, validated: what lsn_resample_span and the stand-alone calls (lsn_front_launch.cc) share
int lsn_resample_plan(const lsn_resample_cfg_t* cfg, lsn::ResamplePlan& plan);
// the same with an antenna map: map null or nof_out = 0 is lsn_resample_plan; else the full cfg, the map's size and ResamplePlan::initMapped's verdict
int lsn_resample_plan_map(const lsn_resample_cfg_t* cfg, const lsn_antenna_map_t* map, lsn::ResamplePlan& plan);

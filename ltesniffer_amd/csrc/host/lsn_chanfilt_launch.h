// lsn_chanfilt_launch.h - the launcher of kernels/chanfilt.hip, the launch record of a cell and the owner of a filter's device tables: the part of the channel
// filter's host side that speaks the HIP runtime's types (lsn_chanfilt.h, the design, does not).
#pragma once
#include <hip/hip_runtime.h>
#include "lsn_chanfilt.h"
#include "lsn_front_source.h"

struct cf32;

// k_chan_fir: what one cell of a launch brings of its own (raw buffer, format, scale and antennas are the recording's).  ChanFirTables::cell alone forms it
struct LsnChanFirCell {
  const float* taps;            // ChanFirTables
  uint32_t L;
  uint64_t w; const cf32* nco;  // nco null: the cell is not translated
  cf32* out;                    // [sample][antenna] cf32, out[0] = y1[out_first]
  int64_t out_first;            // >= 0
  uint64_t n_out;               // 0: the cell takes no part
};

namespace lsn {

// device copy of a filter's taps (padded with zeros to what the kernel's four-tap scalar loads may touch) and, when it mixes, the NCO tables behind them in the
// same allocation: allocated by upload(), freed here.  The twin of ResampleTables (lsn_resample_launch.h)
struct ChanFirTables {
  ChanFirTables() = default;
  ChanFirTables(ChanFirTables&& o) noexcept : d_taps(o.d_taps), d_nco(o.d_nco) { o.d_taps = nullptr; o.d_nco = nullptr; }
  ~ChanFirTables() { if (d_taps) (void)hipFree(d_taps); }
  void upload(const ChanFilter& f, hipStream_t s);   // queued on s and waited for
  // the launch record of y1[out_first, out_first + n_out) of filter f, whose tables these are - the ONE place it is formed
  LsnChanFirCell cell(const ChanFilter& f, cf32* out, int64_t out_first, uint64_t n_out) const
  {
    LsnChanFirCell k;
    k.taps = d_taps; k.L = f.L; k.w = f.tune; k.nco = d_nco; k.out = out; k.out_first = out_first; k.n_out = n_out;
    return k;
  }

private:
  float* d_taps = nullptr;
  const cf32* d_nco = nullptr;
};

}  // namespace lsn

// src (lsn_front_source.h): what a cell reads outside of its window (and in front of sample 0) reads as zeros; a launch out of a ring is k_chan_fir_ring's
void lsn_launch_chan_fir(const LsnFrontSource& src, const LsnChanFirCell* cells, uint32_t n_cells, hipStream_t s);

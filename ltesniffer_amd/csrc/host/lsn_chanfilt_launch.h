// lsn_chanfilt_launch.h - the launcher of kernels/chanfilt.hip and the device copy of a filter: the part of the channel filter's host side that speaks the HIP
// runtime's types (lsn_chanfilt.h, the design, does not).
#pragma once
#include <hip/hip_runtime.h>
#include "lsn_chanfilt.h"

struct cf32;

// device copy of a filter's taps (padded with zeros to what the kernel's four-tap scalar loads may touch) and, when it mixes, the NCO tables behind them in the
// same allocation; the caller frees d_taps
void lsn_chan_fir_upload(const lsn::ChanFilter& f, float*& d_taps, const cf32*& d_nco, hipStream_t s);

// k_chan_fir: what one cell of a launch brings of its own (raw buffer, format, scale and antennas are the recording's)
struct LsnChanFirCell {
  const float* taps;            // lsn_chan_fir_upload
  uint32_t L;
  uint64_t w; const cf32* nco;  // nco null: the cell is not translated
  cf32* out;                    // [sample][antenna] cf32, out[0] = y1[out_first]
  int64_t out_first;            // >= 0
  uint64_t n_out;               // 0: the cell takes no part
};
// raw holds the samples [buf_base, buf_base + buf_len) of the recording; what a cell reads outside of it (and in front of sample 0) reads as zeros.
// ring_samples 0: raw is a linear buffer whose element 0 is sample buf_base.  Otherwise (as LsnResampleSource's): raw is a ring of ring_samples samples per antenna,
// a power of two of at most 2^32 that holds the window (buf_len <= ring_samples), sample n at slot n & (ring_samples - 1); such a launch is k_chan_fir_ring's
void lsn_launch_chan_fir(const void* raw, uint32_t fmt, float scale, int64_t buf_base, uint64_t buf_len, uint32_t nant, uint64_t ring_samples, const LsnChanFirCell* cells,
                         uint32_t n_cells, hipStream_t s);

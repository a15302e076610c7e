// lsn_resample.h - host side of the polyphase resampler (kernels/resample.hip; launchers: lsn_resample_launch.h): the plan of one rate pair - step, start, taps, bank, and the
// tuning word and NCO tables of the mixer in front of the filter - and the 64.64 position arithmetic in 128-bit integers.  Definition: DESIGN.md section 3.1b.
#pragma once
#include <cstdint>
#include <vector>

// no HIP header: the plan is plain host arithmetic, and lsn_cells.cc, which builds on it, stays HIP-free.  What needs the runtime's types - the kernel launchers -
// is declared in lsn_resample_launch.h.
struct cf32;

namespace lsn {

typedef unsigned __int128 u128;

struct ResamplePlan {
  u128 step = 0;       // D = round(rate_in / rate_out * 2^64)
  u128 start = 0;      // P0: position of output sample 0
  uint32_t taps = 0;   // T (even)
  uint32_t span = 0;   // input samples one run of the kernel stages
  std::vector<float> bank;  // [512][T][2]: H[p][j] and H[p + 1][j] - H[p][j], float32 (row 511 reaches phase 512 through its difference)
  uint64_t tune = 0;        // W = floor(center_offset_hz / rate_in * 2^64 + 1/2) mod 2^64: input sample n is rotated by exp(-2 pi j (n W mod 2^64) / 2^64)
  std::vector<float> nco;   // tune != 0: the mixer's tables, [4096] coarse then [1024] fine (re, im), lsn_nco_tables; else empty

  // LSN_SUCCESS, or LSN_ERROR_INVALID_INPUTS when the pair is outside what the filter meets, or the cell at center_offset_hz does not lie inside
  // the recording (accepted range)
  // max_ratio, max_taps: the largest rate_in / rate_out and Kaiser estimate accepted; the defaults are lsn_resample's and the file source's, the carrier
  // scan's narrow-band channel lifts them to 64 and 768
  int init(double rate_in, double rate_out, double passband_hz, uint64_t first_sample, double first_frac, double center_offset_hz, double max_ratio = 4.0,
           uint32_t max_taps = 192);
  static uint64_t tuning(double center_offset_hz, double rate_in);   // W of one offset
  // device copy of bank and nco in one allocation (the caller frees d_bank); d_nco = null when the plan does not mix
  // Stream = hipStream_t, the one instantiation (lsn_resample.cc); a template so that this header names no type of the runtime
  template <class Stream> void upload(float*& d_bank, const cf32*& d_nco, Stream s) const;
  u128 position(uint64_t m) const { return start + (u128)m * step; }
  // input samples [lo, hi) that outputs m0 .. m0 + n - 1 read (lo may be negative: zeros in front of the recording)
  void inputSpan(uint64_t m0, uint64_t n, int64_t& lo, int64_t& hi) const;
  // number of outputs m = 0, 1, ... whose taps all lie in front of input sample in_end
  uint64_t outputsInside(uint64_t in_end) const;
};

}  // namespace lsn

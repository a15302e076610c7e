// lsn_chanfilt.h - host side of the channel filter, stage 1 in front of the resampler (kernels/chanfilt.hip; launcher: lsn_chanfilt_launch.h): the design of
// one filter - half length L, cut-off, the 2L + 1 taps, the mixer's tuning word - its refusals, the input spans it widens, and the span of the intermediate stage 2 reads.  Definition: DESIGN.md section 3.1f.
// No HIP header, like lsn_resample.h: the design is plain host arithmetic and is tested on a machine with no GPU.
#pragma once
#include "../../../include/ltesniffer_amd.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lsn {

constexpr uint32_t kChanMaxL = 512;   // 2L <= 1024: a tile of 1024 outputs stages at most 2048 samples = 16 KB of LDS

struct ChanFilter {
  uint32_t L = 0;            // taps j = -L .. L; 0: no filter
  double fc = 0.0;           // cut-off (B + S) / (2 R), cycles per input sample
  std::vector<float> taps;   // [2L + 1]: g[-L] .. g[L], float32, exactly symmetric
  uint64_t tune = 0;         // W of center_offset_hz (ResamplePlan::tuning): the mixer of DESIGN 3.1b runs while stage 1 stages its input

  // LSN_SUCCESS, or LSN_ERROR_INVALID_INPUTS: a rate, pass band or stop band that is not finite and positive, S <= B, S > R / 2, L > 512, or a cell that does
  // not lie inside the recording (|center_offset_hz| + B > R / 2, the resampler's rule: with the filter on, the resampler itself no longer sees the offset)
  int init(double rate_in, double passband_hz, double stopband_hz, double center_offset_hz);
  // stage 2 reading y1[lo, hi) makes stage 1 read x[lo - L, hi + L)
  void widen(int64_t& lo, int64_t& hi) const { lo -= (int64_t)L; hi += (int64_t)L; }
  // a recording of in_end samples carries y1[n] for n < in_end - L: what stage 2 may read
  uint64_t insideEnd(uint64_t in_end) const { return in_end > L ? in_end - L : 0; }
};

// Stage 2 behind stage 1 (lsn_front_launch.h): a resampler piece that reads the input span [lo, hi) reads y1[lo2, hi2) of its cell's intermediate - the part at or behind
// sample 0 (in front of it the zeros are the resampler's own; a piece wholly in front of the recording: the empty span at 0).  True: it fits an intermediate of cap samples
inline bool chan_mid_span(int64_t lo, int64_t hi, uint64_t cap, int64_t& lo2, int64_t& hi2)
{
  lo2 = std::max<int64_t>(lo, 0);
  hi2 = std::max(hi, lo2);
  return (uint64_t)(hi2 - lo2) <= cap;
}

}  // namespace lsn

// the filter of a lsn_channel_filter_cfg_t, validated: what lsn_channel_filter_span and lsn_channel_filter share
int lsn_channel_filter_plan(const lsn_channel_filter_cfg_t* cfg, lsn::ChanFilter& f);

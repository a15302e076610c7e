// lsn_scan.h - host side of the carrier scan (kernels/scan.hip): the plan - hypotheses, tuning words, the channel filter with the resampler's two caps lifted,
// the geometry of a run - and the decision, all HIP-free; and k_chan_bank's launch record with its launcher.  Definition: DESIGN.md section 3.1d.  The GPU entry
// points are in lsn_scan.cc.
#pragma once
#include "lsn_hip.h"
#include "lsn_resample.h"
#include "lsn_front_source.h"

struct cf32;

namespace lsn {

static constexpr double kScanRateOut = 1.92e6, kScanPassband = 15000.0 * 37.0, kScanMaxRatio = 64.0;
static constexpr uint32_t kScanMaxTaps = 768, kScanN = 128, kScanW5 = 9600;

struct ScanPlan {
  lsn_carrier_scan_cfg_t cfg;          // defaults filled in
  ResamplePlan rs;                     // the channel: rate_in -> 1.92 MS/s, pass band 555 kHz, output 0 at input 0
  std::vector<lsn_carrier_metric_t> hyp;   // k, f_hz, tuning_word
  uint64_t n_chan = 0, n_in = 0;       // channel samples per hypothesis, input samples read
  int init(const lsn_carrier_scan_cfg_t* c);
};

// outputs per workgroup of k_chan_bank and the samples they stage: the largest multiple of 32 up to 256 whose skewed span fits in 64 KB
void chan_geometry(const ResamplePlan& rs, uint32_t& run, uint32_t& span);
// indices into m of the accepted hypotheses, in the order of acceptance
std::vector<uint32_t> scan_decide(const lsn_carrier_scan_cfg_t& cfg, const lsn_carrier_metric_t* m, uint32_t n);

}  // namespace lsn

// k_chan_bank: what a launch brings besides the buffer it reads.  Channel c < nch reads antenna ant0 + c * ant_step, mixes with tunes[c * tune_step] and writes
// out[c * out_stride + m], m < n_out
struct LsnChanBankLaunch {
  uint64_t base_hi, base_lo;   // 64.64 position of output 0 ...
  uint32_t d_hi; uint64_t d_lo;   // ... and the step D
  uint32_t taps, span, run;    // T; samples staged per run of `run` outputs (chan_geometry)
  const float* bank;           // [512][T] (H, dH)
  const uint64_t* tunes; uint32_t tune_step;
  const cf32* nco;             // [4096] coarse then [1024] fine
  uint32_t ant0, ant_step, nch;
  cf32* out; size_t out_stride;
  uint64_t n_out;
};
void lsn_launch_chan_bank(const LsnFrontSource& src, const LsnChanBankLaunch& k, hipStream_t s);   // kernels/scan.hip

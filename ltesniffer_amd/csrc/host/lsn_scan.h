// lsn_scan.h - host side of the carrier scan (kernels/scan.hip): the plan - hypotheses, tuning words, the channel filter with the resampler's two caps lifted,
// the geometry of a run - and the decision.  Definition: DESIGN.md section 3.1d.  Everything here is HIP-free; the GPU entry points are in lsn_scan.cc.
#pragma once
#include "lsn_hip.h"
#include "lsn_resample.h"

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

// lsn_chanfilt.cc - host side of the channel filter (lsn_chanfilt.h): the design, the refusals, the spans, and the entry points that need
// no GPU (lsn_channel_filter_design, lsn_channel_filter_span, lsn_cells_stopbands).  HIP-free host arithmetic; tests/chanfilt_model.py is written from the
// definition in DESIGN, not from this file.
#include "../../../include/ltesniffer_amd.h"
#include "lsn_chanfilt.h"
#include "lsn_resample.h"
#include "lsn_types.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace lsn {

static constexpr double kChanAtten = 80.0;                            // A, dB
static constexpr double kChanBeta = 0.1102 * (kChanAtten - 8.7);      // Kaiser's beta for A > 50

static double chan_i0(double x)
{
  double s = 1.0, t = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; k++) {
    t *= q / ((double)k * (double)k);
    s += t;
    if (t < 1e-20 * s) break;
  }
  return s;
}

int ChanFilter::init(double rate_in, double passband_hz, double stopband_hz, double center_offset_hz)
{
  L = 0; fc = 0.0; taps.clear(); tune = 0;
  if (!(rate_in > 0.0 && rate_in < 1e12) || !(passband_hz > 0.0) || !std::isfinite(stopband_hz)) return LSN_ERROR_INVALID_INPUTS;
  if (!(passband_hz < stopband_hz && stopband_hz <= 0.5 * rate_in)) return LSN_ERROR_INVALID_INPUTS;
  if (!(std::fabs(center_offset_hz) + passband_hz <= 0.5 * rate_in)) return LSN_ERROR_INVALID_INPUTS;   // (NaN and infinity fail here)
  const double width = (stopband_hz - passband_hz) / rate_in;
  const double want = std::ceil((kChanAtten - 7.95) / (14.36 * width) / 2.0);
  if (!(want >= 1.0 && want <= (double)kChanMaxL)) return LSN_ERROR_INVALID_INPUTS;
  L = (uint32_t)want;
  fc = (passband_hz + stopband_hz) / (2.0 * rate_in);
  taps.assign(2 * (size_t)L + 1, 0.0f);
  const double i0b = chan_i0(kChanBeta);
  for (uint32_t j = 0; j <= L; j++) {
    const double u = (double)j / (double)(L + 1), a = M_PI * 2.0 * fc * (double)j;
    const double g = 2.0 * fc * (j ? std::sin(a) / a : 1.0) * chan_i0(kChanBeta * std::sqrt(1.0 - u * u)) / i0b;
    taps[L + j] = taps[L - j] = (float)g;
  }
  tune = ResamplePlan::tuning(center_offset_hz, rate_in);
  return LSN_SUCCESS;
}

}  // namespace lsn

static int chan_cfg_filter(const lsn_channel_filter_cfg_t* cfg, lsn::ChanFilter& f)
{
  if (!cfg || cfg->struct_size != sizeof(lsn_channel_filter_cfg_t)) return LSN_ERROR_INVALID_INPUTS;
  if (cfg->nof_antennas < 1 || cfg->nof_antennas > 8 || !lsn_sample_format(cfg->sample_format, cfg->sample_scale).valid) return LSN_ERROR_INVALID_INPUTS;
  if (cfg->in_base >= (1ull << 62) || cfg->out_first >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  return f.init(cfg->rate_in_hz, cfg->passband_hz, cfg->stopband_hz, cfg->center_offset_hz);
}

// what lsn_channel_filter (lsn_front_launch.cc) validates with
int lsn_channel_filter_plan(const lsn_channel_filter_cfg_t* cfg, lsn::ChanFilter& f) { return chan_cfg_filter(cfg, f); }

extern "C" {

int lsn_channel_filter_design(double rate_in_hz, double passband_hz, double stopband_hz, lsn_channel_filter_design_t* out, float* taps, uint32_t cap)
{
  if (!out || out->struct_size != sizeof(lsn_channel_filter_design_t)) return LSN_ERROR_INVALID_INPUTS;
  lsn::ChanFilter f;
  const int r = f.init(rate_in_hz, passband_hz, stopband_hz, 0.0);
  if (r != LSN_SUCCESS) return r;
  if (taps && cap < f.taps.size()) return LSN_ERROR_INVALID_INPUTS;
  out->half_len = f.L; out->nof_taps = (uint32_t)f.taps.size(); out->reserved = 0; out->cutoff = f.fc;
  if (taps) memcpy(taps, f.taps.data(), f.taps.size() * sizeof(float));
  return LSN_SUCCESS;
}

int lsn_channel_filter_span(const lsn_channel_filter_cfg_t* cfg, uint64_t n_out, uint64_t in_end, lsn_resample_span_t* out)
{
  lsn::ChanFilter f;
  const int r = chan_cfg_filter(cfg, f);
  if (r != LSN_SUCCESS || !out) return r != LSN_SUCCESS ? r : LSN_ERROR_INVALID_INPUTS;
  if (n_out >= (1ull << 40) || in_end >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  memset(out, 0, sizeof(*out));
  out->taps = 2 * f.L + 1;
  out->in_lo = (int64_t)cfg->out_first; out->in_hi = (int64_t)(cfg->out_first + n_out);
  f.widen(out->in_lo, out->in_hi);
  const uint64_t inside = f.insideEnd(in_end);
  out->max_out = inside > cfg->out_first ? inside - cfg->out_first : 0;
  return LSN_SUCCESS;
}

int lsn_cells_stopbands(const double* carrier_hz, const uint32_t* nof_prb, uint32_t n, double rate_in_hz, double* stopband_hz)
{
  if (!carrier_hz || !nof_prb || !stopband_hz || n < 1 || n > LSN_FILE_MAX_CELLS || !(rate_in_hz > 0.0 && rate_in_hz < 1e12)) return LSN_ERROR_INVALID_INPUTS;
  auto edge = [&](uint32_t i) { return 15000.0 * (6.0 * (double)nof_prb[i] + 1.0); };
  for (uint32_t i = 0; i < n; i++)
    if (!std::isfinite(carrier_hz[i]) || !nof_prb[i] || nof_prb[i] > 110) return LSN_ERROR_INVALID_INPUTS;
  double s[LSN_FILE_MAX_CELLS];
  for (uint32_t i = 0; i < n; i++) {
    double best = 0.0;
    bool have = false;
    for (uint32_t j = 0; j < n; j++) {
      if (j == i) continue;
      const double d = std::fabs(carrier_hz[j] - carrier_hz[i]) - edge(j);
      best = have ? std::min(best, d) : d;
      have = true;
    }
    s[i] = 0.0;
    if (!have) continue;
    best = std::min(best, 0.5 * rate_in_hz);
    if (!(best > edge(i))) continue;
    lsn::ChanFilter f;
    if (f.init(rate_in_hz, edge(i), best, 0.0) != LSN_SUCCESS) return LSN_ERROR_INVALID_INPUTS;   // (L above 512: the neighbour is too close for this filter)
    s[i] = best;
  }
  memcpy(stopband_hz, s, n * sizeof(double));
  return LSN_SUCCESS;
}

}  // extern "C"

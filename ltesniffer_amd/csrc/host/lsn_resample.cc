// lsn_resample.cc - host side of the polyphase resampler: the plan of a rate pair (step and start in 64.64 fixed point, formed in 128-bit
// integers; number of taps; the bank of 512 phases; the tuning word and tables of the mixer), ResampleTables, the owner of a cell's device copies of them, and
// lsn_resample_span (the stand-alone calls that launch: lsn_front_launch.cc).
// The filter is DESIGN.md section 3.1b, restated there as a formula; tests/resample_model.py is written from that formula, not from this file.
// Product code: nothing from oracle/ is included or linked.
#include "lsn_hip.h"
#include "../kernels/lsn_dev.h"
#include "lsn_resample_launch.h"
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

namespace lsn {

static constexpr double kAtten = 80.0;                          // design attenuation A of the Kaiser window, dB
static constexpr double kBeta = 0.1102 * (kAtten - 8.7);        // Kaiser's beta for A > 50
static constexpr uint32_t kPhases = 512;

static double bessel_i0(double x)
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

// W = floor(center_offset_hz / rate_in * 2^64 + 1/2) mod 2^64, the quotient of the two doubles taken exactly as for D: |quotient| <= 1/2, so ec <= ea and
// mc << sw stays below 2^118
uint64_t ResamplePlan::tuning(double center_offset_hz, double rate_in)
{
  if (center_offset_hz == 0.0) return 0;
  int ea = 0, ec = 0;
  const uint64_t ma = (uint64_t)std::ldexp(std::frexp(rate_in, &ea), 53), mc = (uint64_t)std::ldexp(std::frexp(std::fabs(center_offset_hz), &ec), 53);
  const int sw = 64 + ec - ea;
  if (sw < -1) return 0;   // below that the quotient times 2^64 is under 1/2 in magnitude: W = 0
  const __int128 num = (__int128)((u128)mc << std::max(sw, 0)) * (center_offset_hz < 0.0 ? -2 : 2), den = (__int128)((u128)ma << std::max(-sw, 0)) * 2;
  const __int128 a = num + den / 2;   // floor(a / den) = floor(quotient 2^64 + 1/2)
  return (uint64_t)(a >= 0 ? a / den : -((-a + den - 1) / den));
}

int ResamplePlan::init(double rate_in, double rate_out, double passband_hz, uint64_t first_sample, double first_frac, double center_offset_hz, double max_ratio,
                       uint32_t max_taps)
{
  if (!(rate_in > 0.0 && rate_in < 1e12) || !(rate_out > 0.0 && rate_out < 1e12)) return LSN_ERROR_INVALID_INPUTS;
  if (!(first_frac >= 0.0 && first_frac < 1.0) || first_sample >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  const double ratio = rate_in / rate_out;
  if (!(ratio >= 1.0 / 65536.0)) return LSN_ERROR_INVALID_INPUTS;
  if (!(ratio <= max_ratio)) {   // the wide-ratio run (accepted range)
    if (!(ratio <= kWideMaxRatio && rate_in <= kWideMaxRateIn && rate_out >= kWideMinRateOut)) return LSN_ERROR_INVALID_INPUTS;
    max_taps = kWideMaxTaps;
  }
  const double lo_rate = std::min(rate_in, rate_out), rho = std::max(1.0, ratio);
  if (passband_hz == 0.0) passband_hz = 0.44 * lo_rate;
  if (!(passband_hz > 0.0)) return LSN_ERROR_INVALID_INPUTS;
  const double width = (lo_rate - 2.0 * passband_hz) / rate_in;   // transition band [B, min(rate) - B], in cycles per input sample
  if (!(width > 0.0)) return LSN_ERROR_INVALID_INPUTS;
  if (!(std::fabs(center_offset_hz) + passband_hz <= 0.5 * rate_in)) return LSN_ERROR_INVALID_INPUTS;   // the cell lies inside the recording (NaN and infinity fail here)
  const double want = (kAtten - 7.95) / (14.36 * width) + 1.0;    // Kaiser's estimate of the filter length
  if (!(want <= (double)max_taps)) return LSN_ERROR_INVALID_INPUTS;
  taps = std::max(4u, 2u * (uint32_t)std::ceil(want / 2.0));
  // D = round(rate_in / rate_out * 2^64), exactly: the two doubles are integers ma 2^(ea - 53), mb 2^(eb - 53)
  int ea = 0, eb = 0;
  const uint64_t ma = (uint64_t)std::ldexp(std::frexp(rate_in, &ea), 53), mb = (uint64_t)std::ldexp(std::frexp(rate_out, &eb), 53);
  const int sh = 65 + ea - eb;   // 47 .. 68 for ratios up to 4, up to 72 for the carrier scan's 64: ma << sh stays below 2^125
  if (sh < 0 || sh > 72) return LSN_ERROR_INVALID_INPUTS;
  step = (((u128)ma << sh) + (u128)mb) / ((u128)mb << 1);
  if (step == 0) return LSN_ERROR_INVALID_INPUTS;
  start = ((u128)first_sample << 64) + (u128)(uint64_t)std::ldexp(first_frac, 64);
  tune = tuning(center_offset_hz, rate_in);
  map_nout = 0;
  nco.clear();
  if (tune) {
    nco.resize((4096 + 1024) * 2);
    lsn_nco_tables((cf32*)nco.data(), (cf32*)nco.data() + 4096);
  }
  grp = groupOf(step);
  run = runOf(grp);
  span = spanAt(step);
  // bank: H[p][j] = h(j - T/2 + 1 - p / 512), h(t) = sinc(t / rho) / rho * I0(beta sqrt(1 - (2 t / T)^2)) / I0(beta)
  const double i0b = bessel_i0(kBeta), half = 0.5 * (double)taps;
  auto h = [&](double t) {
    const double u = t / half;
    if (u < -1.0 || u > 1.0) return 0.0;
    const double w = bessel_i0(kBeta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b, a = M_PI * t / rho;
    return (a == 0.0 ? 1.0 : std::sin(a) / a) / rho * w;
  };
  bank.assign((size_t)kPhases * taps * 2, 0.0f);
  for (uint32_t p = 0; p < kPhases; p++)
    for (uint32_t j = 0; j < taps; j++) {
      const double t0 = (double)j - half + 1.0 - (double)p / kPhases, t1 = (double)j - half + 1.0 - (double)(p + 1) / kPhases;
      const double h0 = h(t0), h1 = h(t1);
      bank[((size_t)p * taps + j) * 2] = (float)h0;
      bank[((size_t)p * taps + j) * 2 + 1] = (float)(h1 - h0);
    }
  return LSN_SUCCESS;
}

int ResamplePlan::initMapped(double rate_in, double rate_out, double passband_hz, uint64_t first_sample, double first_frac, double center_offset_hz, uint32_t nof_in,
                             uint32_t nof_out, const uint32_t* src, const double* offset_hz)
{
  if (nof_out < 1 || nof_out > LSN_RS_MAP_MAX_OUT || !src || !offset_hz) return LSN_ERROR_INVALID_INPUTS;
  for (uint32_t a = 0; a < nof_out; a++) if (src[a] >= nof_in) return LSN_ERROR_INVALID_INPUTS;
  const int r = init(rate_in, rate_out, passband_hz, first_sample, first_frac, 0.0);
  if (r != LSN_SUCCESS) return r;
  if (passband_hz == 0.0) passband_hz = 0.44 * std::min(rate_in, rate_out);   // init's default
  bool mixes = false;
  for (uint32_t a = 0; a < nof_out; a++) {
    const double f = center_offset_hz + offset_hz[a];
    if (!(std::fabs(f) + passband_hz <= 0.5 * rate_in)) return LSN_ERROR_INVALID_INPUTS;   // the output lies inside the recording (NaN and infinity fail here)
    map_src[a] = src[a];
    map_w[a] = tuning(f, rate_in);
    mixes = mixes || map_w[a] != 0;
  }
  map_nout = nof_out;
  if (mixes) {
    nco.resize((4096 + 1024) * 2);
    lsn_nco_tables((cf32*)nco.data(), (cf32*)nco.data() + 4096);
  }
  return LSN_SUCCESS;
}

void ResampleTables::upload(const ResamplePlan& p, hipStream_t s)
{
  HIP_CHECK(hipMalloc((void**)&d_bank, (p.bank.size() + p.nco.size()) * sizeof(float)));
  HIP_CHECK(hipMemcpyAsync(d_bank, p.bank.data(), p.bank.size() * sizeof(float), hipMemcpyHostToDevice, s));
  d_nco = nullptr;
  if (!p.nco.empty()) {
    HIP_CHECK(hipMemcpyAsync(d_bank + p.bank.size(), p.nco.data(), p.nco.size() * sizeof(float), hipMemcpyHostToDevice, s));
    d_nco = (const cf32*)(d_bank + p.bank.size());
  }
}

void ResampleTables::rotation(float offset_freq_hz, uint32_t sflen, double fs)
{
  if (offset_freq_hz == 0.0f) return;
  std::vector<cf32> rot(sflen);
  for (uint32_t n = 0; n < sflen; n++) {
    const double a = -2.0 * M_PI * (double)offset_freq_hz * (double)n / fs;
    rot[n] = {(float)std::cos(a), (float)std::sin(a)};
  }
  HIP_CHECK(hipMalloc((void**)&d_rot, sflen * sizeof(cf32)));
  HIP_CHECK(hipMemcpy(d_rot, rot.data(), sflen * sizeof(cf32), hipMemcpyHostToDevice));
}

ResampleTables::~ResampleTables()
{
  if (d_rot) (void)hipFree(d_rot);
  if (d_bank) (void)hipFree(d_bank);
}

void ResamplePlan::inputSpan(uint64_t m0, uint64_t n, int64_t& lo, int64_t& hi) const
{
  const int64_t half = (int64_t)taps / 2;
  lo = (int64_t)(uint64_t)(position(m0) >> 64) - half + 1;
  hi = (int64_t)(uint64_t)(position(m0 + (n ? n - 1 : 0)) >> 64) + half + 1;
}

uint64_t ResamplePlan::outputsInside(uint64_t in_end) const
{
  const uint64_t half = taps / 2;
  if (in_end <= half || in_end >= (1ull << 62)) return 0;
  const u128 lim = (u128)(in_end - half) << 64;   // positions below lim read no sample at or behind in_end
  if (start >= lim) return 0;
  const u128 n = (lim - 1 - start) / step + 1;
  return n > (u128)(1ull << 62) ? (1ull << 62) : (uint64_t)n;
}

}  // namespace lsn

int lsn_resample_plan(const lsn_resample_cfg_t* cfg, lsn::ResamplePlan& plan)
{
  // two sizes are known: the struct up to passband_hz (center_offset_hz reads as 0) and the whole struct
  if (!cfg || (cfg->struct_size != offsetof(lsn_resample_cfg_t, center_offset_hz) && cfg->struct_size != sizeof(lsn_resample_cfg_t))) return LSN_ERROR_INVALID_INPUTS;
  const double center = cfg->struct_size == sizeof(lsn_resample_cfg_t) ? cfg->center_offset_hz : 0.0;
  if (cfg->nof_antennas < 1 || cfg->nof_antennas > 8 || !lsn_sample_format(cfg->sample_format, cfg->sample_scale).valid) return LSN_ERROR_INVALID_INPUTS;
  return plan.init(cfg->rate_in_hz, cfg->rate_out_hz, cfg->passband_hz, cfg->first_sample, cfg->first_frac, center);
}

int lsn_resample_plan_map(const lsn_resample_cfg_t* cfg, const lsn_antenna_map_t* map, lsn::ResamplePlan& plan)
{
  if (!map || !map->nof_out) return lsn_resample_plan(cfg, plan);
  if (!cfg || cfg->struct_size != sizeof(lsn_resample_cfg_t) || map->struct_size != sizeof(lsn_antenna_map_t)) return LSN_ERROR_INVALID_INPUTS;
  if (cfg->nof_antennas < 1 || cfg->nof_antennas > 8 || !lsn_sample_format(cfg->sample_format, cfg->sample_scale).valid) return LSN_ERROR_INVALID_INPUTS;
  return plan.initMapped(cfg->rate_in_hz, cfg->rate_out_hz, cfg->passband_hz, cfg->first_sample, cfg->first_frac, cfg->center_offset_hz, cfg->nof_antennas, map->nof_out,
                         map->src_antenna, map->offset_hz);
}

extern "C" {

int lsn_resample_span(const lsn_resample_cfg_t* cfg, uint64_t n_out, uint64_t in_end, lsn_resample_span_t* out)
{
  lsn::ResamplePlan plan;
  const int r = lsn_resample_plan(cfg, plan);
  if (r != LSN_SUCCESS || !out) return r != LSN_SUCCESS ? r : LSN_ERROR_INVALID_INPUTS;
  if (cfg->out_first >= (1ull << 40) || n_out >= (1ull << 40)) return LSN_ERROR_INVALID_INPUTS;
  memset(out, 0, sizeof(*out));
  out->taps = plan.taps;
  plan.inputSpan(cfg->out_first, n_out, out->in_lo, out->in_hi);
  const uint64_t inside = plan.outputsInside(in_end);
  out->max_out = inside > cfg->out_first ? inside - cfg->out_first : 0;
  return LSN_SUCCESS;
}

}  // extern "C"

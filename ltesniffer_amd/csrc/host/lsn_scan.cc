// lsn_scan.cc - carrier scan: which LTE carriers does a wideband recording hold, and where.  Host side: the plan (hypotheses on the
// raster, their tuning words, the 1.92 MS/s channel filter = the resampler's plan with its two caps lifted), the batches over k_chan_bank -> k_pss_corr ->
// k_scan_peaks (kernels/scan.hip, stage_sync.hip), the decision, and the cell search on every accepted carrier's channel.  lsn_carrier_channel hands out the
// channel of one offset through the same kernel.  antenna = LSN_SCAN_ALL_ANTENNAS: a channel per (hypothesis, antenna), k_pss_corr_ant adds the antennas'
// correlations (kernels/sync_ant.hip), the accepted carriers go through the cell search over all antennas.  Product code: no CPU fallback, nothing from oracle/ is included or linked.
#include "lsn_hip.h"
#include "../kernels/lsn_dev.h"
#include "lsn_scan.h"
#include "lsn_resample_launch.h"
#include "lsn_sync_ant.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <fcntl.h>
#include <unistd.h>
#include <vector>

void lsn_launch_scan_peaks(const float* C, size_t c_stride, uint32_t W5, uint32_t nroots, uint32_t nch, void* out, hipStream_t s);
void lsn_launch_pss_corr_bank(const cf32* x, size_t x_stride, const cf32* p, uint32_t N, uint32_t W5, uint32_t P, uint32_t nroots, float* C, size_t c_stride, uint32_t nch,
                              hipStream_t s);

namespace lsn {

void pss_replica_d(uint32_t n_id_2, uint32_t N, double rot_hz, double* p);   // lsn_sync.cc
int cell_search(int device, const cf32* iq, bool on_device, uint64_t nsamples, uint32_t nof_prb, int rates, const lsn_cell_search_cfg_t& cfg, lsn_cell_search_t& out,
                float* corr_out);

static constexpr size_t kScanScratch = (size_t)256 << 20;   // device bytes for the channels, correlations and peaks of one batch

int ScanPlan::init(const lsn_carrier_scan_cfg_t* c)
{
  if (!c || c->struct_size != sizeof(lsn_carrier_scan_cfg_t)) return LSN_ERROR_INVALID_INPUTS;
  cfg = *c;
  if (cfg.nof_periods == 0) cfg.nof_periods = 2;
  if (cfg.raster_hz == 0.0) cfg.raster_hz = 100e3;
  if (cfg.min_spacing_hz == 0.0) cfg.min_spacing_hz = 1.4e6;
  if (cfg.threshold == 0.0f) cfg.threshold = 20.0f;
  if (cfg.nof_periods > 16 || !(cfg.raster_hz > 0.0 && cfg.raster_hz < 1e12) || !std::isfinite(cfg.raster_offset_hz) || !std::isfinite(cfg.f_lo_hz) ||
      !std::isfinite(cfg.f_hi_hz) || cfg.f_lo_hz > cfg.f_hi_hz || !(cfg.min_spacing_hz > 0.0) || !(cfg.threshold > 0.0f))
    return LSN_ERROR_INVALID_INPUTS;
  const double rate = cfg.rate_in_hz;
  if (!(rate >= kScanRateOut && rate <= kScanMaxRatio * kScanRateOut)) return LSN_ERROR_INVALID_INPUTS;
  const int r = rs.init(rate, kScanRateOut, kScanPassband, 0, 0.0, 0.0, kScanMaxRatio, kScanMaxTaps);
  if (r != LSN_SUCCESS) return r;
  rs.nco.resize((4096 + 1024) * 2);
  lsn_nco_tables((cf32*)rs.nco.data(), (cf32*)rs.nco.data() + 4096);
  // hypotheses: every integer k whose f_k passes the rule, evaluated on the double f_k itself; the bracket below is two raster steps wider than the rule
  const bool narrow = !(cfg.f_lo_hz == 0.0 && cfg.f_hi_hz == 0.0);
  const double edge = 0.5 * rate - kScanPassband;
  double lo = -edge, hi = edge;
  if (narrow) { lo = std::max(lo, cfg.f_lo_hz); hi = std::min(hi, cfg.f_hi_hz); }
  hyp.clear();
  if (hi >= lo) {
    const double ka = std::floor((lo - cfg.raster_offset_hz) / cfg.raster_hz) - 2.0, kb = std::ceil((hi - cfg.raster_offset_hz) / cfg.raster_hz) + 2.0;
    if (!(std::fabs(ka) < 1e9 && std::fabs(kb) < 1e9) || kb - ka > (double)LSN_SCAN_MAX_HYPOTHESES + 8.0) return LSN_ERROR_INVALID_INPUTS;
    for (int64_t k = (int64_t)ka; k <= (int64_t)kb; k++) {
      const double f = (double)k * cfg.raster_hz + cfg.raster_offset_hz;
      if (!(std::fabs(f) + kScanPassband <= 0.5 * rate)) continue;
      if (narrow && !(f >= cfg.f_lo_hz && f <= cfg.f_hi_hz)) continue;
      lsn_carrier_metric_t m;
      std::memset(&m, 0, sizeof m);
      m.k = (int32_t)k;
      m.f_hz = f;
      m.tuning_word = ResamplePlan::tuning(f, rate);
      hyp.push_back(m);
    }
  }
  if (hyp.empty() || hyp.size() > LSN_SCAN_MAX_HYPOTHESES) return LSN_ERROR_INVALID_INPUTS;
  n_chan = (uint64_t)(cfg.nof_periods + 1) * kScanW5 + kScanN;
  int64_t a, b;
  rs.inputSpan(0, n_chan, a, b);
  n_in = (uint64_t)b;
  return LSN_SUCCESS;
}

void chan_geometry(const ResamplePlan& rs, uint32_t& run, uint32_t& span)
{
  for (run = 256;; run -= 32) {
    span = (uint32_t)(((u128)run * rs.step) >> 64) + rs.taps + 2;
    if (((size_t)span + (span >> 5) + 1) * 8 <= 64 * 1024 || run == 32) return;
  }
}

std::vector<uint32_t> scan_decide(const lsn_carrier_scan_cfg_t& cfg, const lsn_carrier_metric_t* m, uint32_t n)
{
  std::vector<uint32_t> cand, acc;
  // the floor on the peak itself: threshold times P / N, what the mean of C is on a white channel.  A channel whose pass band is empty while its transition
  // band holds a strong neighbour has a mean far below that (the neighbour fills the energy every C is divided by) and a p2avg of 20 .. 160 on nothing
  const float floor_peak = cfg.threshold * (float)cfg.nof_periods / (float)kScanN;
  for (uint32_t i = 0; i < n; i++)
    if (m[i].p2avg >= cfg.threshold && m[i].peak >= floor_peak) cand.push_back(i);
  std::sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) {
    if (m[a].p2avg != m[b].p2avg) return m[a].p2avg > m[b].p2avg;
    const double fa = std::fabs(m[a].f_hz), fb = std::fabs(m[b].f_hz);
    if (fa != fb) return fa < fb;
    return m[a].k < m[b].k;
  });
  for (uint32_t i : cand) {
    bool keep = true;
    for (uint32_t j : acc)
      if (std::fabs(m[i].f_hz - m[j].f_hz) < cfg.min_spacing_hz) { keep = false; break; }
    if (keep) acc.push_back(i);
  }
  return acc;
}

namespace {
struct ScanPeak { double sum; float peak; uint32_t lag; uint32_t pad[2]; };   // LsnScanPeak of scan.hip
static_assert(sizeof(ScanPeak) == 24, "24 bytes per (hypothesis, root)");
}  // namespace

static int carrier_scan(int device, const void* in, bool in_on_device, uint64_t n_in, const lsn_carrier_scan_cfg_t* ucfg, lsn_carrier_t* carriers_out, uint32_t cap,
                        lsn_carrier_metric_t* metric_out)
{
  ScanPlan sp;
  const int r = sp.init(ucfg);
  if (r != LSN_SUCCESS) return r;
  const lsn_carrier_scan_cfg_t& cfg = sp.cfg;
  const LsnSampleFormat sfm = lsn_sample_format(cfg.sample_format, cfg.sample_scale);
  const bool all = cfg.antenna == LSN_SCAN_ALL_ANTENNAS;
  if (!in || !sfm.valid || cfg.nof_antennas < 1 || cfg.nof_antennas > 8 || (!all && cfg.antenna >= cfg.nof_antennas) || n_in < sp.n_in || (cap && !carriers_out))
    return LSN_ERROR_INVALID_INPUTS;
  if (!have_device(device)) return LSN_ERROR_NO_DEVICE;
  HIP_CHECK(hipSetDevice(device));
  OwnedStream st;
  const ResamplePlan& rs = sp.rs;
  const uint32_t H = (uint32_t)sp.hyp.size(), P = cfg.nof_periods, N = kScanN, W5 = kScanW5;
  const size_t smp = (size_t)sfm.bytes * cfg.nof_antennas, nch = (size_t)sp.n_chan;
  uint32_t run, span;
  chan_geometry(rs, run, span);

  DevBuf bin, btune, brep, bchan, bcorr, bpeak;
  ResampleTables tb;
  const void* d_in = in;
  if (!in_on_device) {
    d_in = bin.alloc<uint8_t>(sp.n_in * smp);
    HIP_CHECK(hipMemcpyAsync((void*)d_in, in, sp.n_in * smp, hipMemcpyHostToDevice, st.s));
  }
  tb.upload(rs, st.s);
  std::vector<uint64_t> tunes(H);
  for (uint32_t i = 0; i < H; i++) tunes[i] = sp.hyp[i].tuning_word;
  uint64_t* d_tune = btune.alloc<uint64_t>(H);
  HIP_CHECK(hipMemcpyAsync(d_tune, tunes.data(), H * sizeof(uint64_t), hipMemcpyHostToDevice, st.s));
  std::vector<cf32> rep((size_t)3 * N);
  {
    std::vector<double> pd(2 * (size_t)N);
    for (uint32_t q = 0; q < 3; q++) {
      pss_replica_d(q, N, 0.0, pd.data());
      for (uint32_t n = 0; n < N; n++) rep[(size_t)q * N + n] = {(float)pd[2 * n], (float)pd[2 * n + 1]};
    }
  }
  cf32* d_rep = brep.alloc<cf32>(rep.size());
  HIP_CHECK(hipMemcpyAsync(d_rep, rep.data(), rep.size() * sizeof(cf32), hipMemcpyHostToDevice, st.s));

  // batches: the scratch of one batch stays under kScanScratch whatever H is; a hypothesis has A channels (one per scanned antenna) and one correlation
  const uint32_t A = all ? cfg.nof_antennas : 1;
  const size_t per = A * nch * sizeof(cf32) + (size_t)3 * W5 * sizeof(float) + 3 * sizeof(ScanPeak);
  const uint32_t batch = (uint32_t)std::min<size_t>(std::min<size_t>(H, 65535), std::max<size_t>(1, kScanScratch / per));
  const size_t ant_stride = (size_t)batch * nch;   // the bank is [antenna][hypothesis of the batch][sample]
  cf32* d_chan = bchan.alloc<cf32>(A * ant_stride);
  float* d_corr = bcorr.alloc<float>((size_t)batch * 3 * W5);
  ScanPeak* d_peak = bpeak.alloc<ScanPeak>((size_t)batch * 3);
  std::vector<ScanPeak> peaks((size_t)batch * 3);
  std::vector<lsn_carrier_metric_t> metric = sp.hyp;
  // hypotheses h0 .. h0 + n - 1, one channel each per scanned antenna (a launch per antenna: all its channels read one antenna); output 0 at input 0
  auto channels = [&](uint32_t h0, uint32_t n) {
    for (uint32_t a = 0; a < A; a++)
      lsn_launch_chan_bank({d_in, cfg.sample_format, sfm.scale, 0, sp.n_in, cfg.nof_antennas, 0},
                           {0, 0, (uint32_t)(rs.step >> 64), (uint64_t)rs.step, rs.taps, span, run, tb.d_bank, d_tune + h0, 1, tb.d_nco, all ? a : cfg.antenna, 0, n,
                            d_chan + a * ant_stride, nch, nch},
                           st.s);
  };
  for (uint32_t h0 = 0; h0 < H; h0 += batch) {
    const uint32_t n = std::min(batch, H - h0);
    channels(h0, n);
    if (all) lsn_launch_pss_corr_ant(d_chan, nch, ant_stride, A, d_rep, N, W5, P, 3, 0, W5, d_corr, (size_t)3 * W5, n, st.s);
    else lsn_launch_pss_corr_bank(d_chan, nch, d_rep, N, W5, P, 3, d_corr, (size_t)3 * W5, n, st.s);
    lsn_launch_scan_peaks(d_corr, (size_t)3 * W5, W5, 3, n, d_peak, st.s);
    HIP_CHECK(hipMemcpyAsync(peaks.data(), d_peak, (size_t)n * 3 * sizeof(ScanPeak), hipMemcpyDeviceToHost, st.s));
    HIP_CHECK(hipStreamSynchronize(st.s));
    for (uint32_t i = 0; i < n; i++) {
      // the first maximum in (root, lag) order; the mean of the winning root, summed in double (lsn_sync.cc)
      const ScanPeak* pk = &peaks[(size_t)i * 3];
      uint32_t br = 0;
      for (uint32_t q = 1; q < 3; q++)
        if (pk[q].peak > pk[br].peak) br = q;
      const double mean = pk[br].sum / (double)W5;
      lsn_carrier_metric_t& m = metric[h0 + i];
      m.root = br;
      m.lag = pk[br].lag;
      m.peak = pk[br].peak;
      m.p2avg = mean > 0.0 ? (float)((double)pk[br].peak / mean) : 0.0f;
    }
  }
  if (metric_out) std::memcpy(metric_out, metric.data(), (size_t)H * sizeof(lsn_carrier_metric_t));
  const std::vector<uint32_t> acc = scan_decide(cfg, metric.data(), H);
  lsn_cell_search_cfg_t cs;
  cs.nof_periods = P;
  cs.force_n_id_2 = -1;
  cs.threshold = cfg.threshold;
  for (size_t i = 0; i < acc.size() && i < cap; i++) {
    const lsn_carrier_metric_t& m = metric[acc[i]];
    lsn_carrier_t& c = carriers_out[i];
    std::memset(&c, 0, sizeof c);
    c.center_offset_hz = m.f_hz;
    c.k = m.k;
    c.scan_p2avg = m.p2avg;
    c.scan_root = m.root;
    c.scan_lag = m.lag;
    channels(acc[i], 1);
    HIP_CHECK(hipStreamSynchronize(st.s));
    const int rc = all ? cell_search_ant(device, d_chan, true, sp.n_chan, ant_stride, A, kSearchAntCap, 6, LSN_RATES_3GPP, cs, c.search, nullptr, nullptr)
                       : cell_search(device, d_chan, true, sp.n_chan, 6, LSN_RATES_3GPP, cs, c.search, nullptr);
    if (rc < 0) return rc;
  }
  return (int)acc.size();
}

static int channel_plan(const lsn_carrier_channel_cfg_t* cfg, ResamplePlan& plan)
{
  if (!cfg || cfg->struct_size != sizeof(lsn_carrier_channel_cfg_t)) return LSN_ERROR_INVALID_INPUTS;
  if (cfg->nof_antennas < 1 || cfg->nof_antennas > 8 || !lsn_sample_format(cfg->sample_format, cfg->sample_scale).valid) return LSN_ERROR_INVALID_INPUTS;
  if (!(cfg->rate_in_hz >= kScanRateOut && cfg->rate_in_hz <= kScanMaxRatio * kScanRateOut)) return LSN_ERROR_INVALID_INPUTS;
  if (cfg->out_first >= (1ull << 40) || cfg->in_base >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  const int r = plan.init(cfg->rate_in_hz, kScanRateOut, kScanPassband, cfg->first_sample, cfg->first_frac, cfg->center_offset_hz, kScanMaxRatio, kScanMaxTaps);
  if (r != LSN_SUCCESS) return r;
  plan.nco.resize((4096 + 1024) * 2);   // the channel always goes through the mixer (W = 0 multiplies by one): one kernel, one value per sample
  lsn_nco_tables((cf32*)plan.nco.data(), (cf32*)plan.nco.data() + 4096);
  return LSN_SUCCESS;
}

static int carrier_channel(int device, const void* in, bool in_on_device, uint64_t n_in, const lsn_carrier_channel_cfg_t* cfg, float* out, bool out_on_device, uint64_t n_out)
{
  ResamplePlan plan;
  const int r = channel_plan(cfg, plan);
  if (r != LSN_SUCCESS) return r;
  if (!n_out) return LSN_SUCCESS;
  if (!in || !out || n_out >= (1ull << 32) || n_in >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  int64_t lo, hi;
  plan.inputSpan(cfg->out_first, n_out, lo, hi);
  if (hi >= (int64_t)1 << 62) return LSN_ERROR_INVALID_INPUTS;
  const LsnWindowNeed need = lsn_window_holds(cfg->in_base, n_in, lo, hi);
  if (!need.ok) return LSN_ERROR_INVALID_INPUTS;
  if (!have_device(device)) return LSN_ERROR_NO_DEVICE;
  const uint32_t nant = cfg->nof_antennas;
  const LsnSampleFormat sfm = lsn_sample_format(cfg->sample_format, cfg->sample_scale);
  const size_t smp = (size_t)sfm.bytes * nant;
  const uint8_t* src = (const uint8_t*)in + ((uint64_t)need.lo - cfg->in_base) * smp;
  HIP_CHECK(hipSetDevice(device));
  OwnedStream st;
  DevBuf bin, btune, bout;
  ResampleTables tb;
  tb.upload(plan, st.s);
  uint64_t* d_tune = btune.alloc<uint64_t>(1);
  HIP_CHECK(hipMemcpyAsync(d_tune, &plan.tune, sizeof(uint64_t), hipMemcpyHostToDevice, st.s));
  const void* raw = src;
  if (!in_on_device) {
    raw = bin.alloc<uint8_t>(need.len * smp);
    if (need.len) HIP_CHECK(hipMemcpyAsync((void*)raw, src, need.len * smp, hipMemcpyHostToDevice, st.s));
  }
  cf32* dst = (cf32*)out;
  const size_t out_bytes = (size_t)n_out * nant * sizeof(cf32);
  if (!out_on_device) dst = bout.alloc<cf32>((size_t)n_out * nant);
  uint32_t run, span;
  chan_geometry(plan, run, span);
  const u128 base = plan.position(cfg->out_first);
  // one tuning word, a channel per antenna
  lsn_launch_chan_bank({raw, cfg->sample_format, sfm.scale, need.lo, need.len, nant, 0},
                       {(uint64_t)(base >> 64), (uint64_t)base, (uint32_t)(plan.step >> 64), (uint64_t)plan.step, plan.taps, span, run, tb.d_bank, d_tune, 0, tb.d_nco, 0, 1, nant, dst,
                        n_out, n_out},
                       st.s);
  if (!out_on_device) HIP_CHECK(hipMemcpyAsync(out, dst, out_bytes, hipMemcpyDeviceToHost, st.s));
  HIP_CHECK(hipStreamSynchronize(st.s));
  return LSN_SUCCESS;
}

}  // namespace lsn

extern "C" {

int lsn_carrier_scan_plan(const lsn_carrier_scan_cfg_t* cfg, lsn_carrier_scan_plan_t* out, lsn_carrier_metric_t* hyp, uint32_t cap, float* bank_out)
{
  return lsn::guarded([&]() -> int {
    lsn::ScanPlan sp;
    const int r = sp.init(cfg);
    if (r != LSN_SUCCESS) return r;
    if (!out || (hyp && cap < sp.hyp.size())) return LSN_ERROR_INVALID_INPUTS;
    std::memset(out, 0, sizeof *out);
    out->nof_hypotheses = (uint32_t)sp.hyp.size();
    out->taps = sp.rs.taps;
    out->nof_periods = sp.cfg.nof_periods;
    out->nof_channel_samples = sp.n_chan;
    out->nof_input_samples = sp.n_in;
    if (hyp) std::memcpy(hyp, sp.hyp.data(), sp.hyp.size() * sizeof(lsn_carrier_metric_t));
    if (bank_out) std::memcpy(bank_out, sp.rs.bank.data(), sp.rs.bank.size() * sizeof(float));
    return LSN_SUCCESS;
  });
}

int lsn_carrier_scan_decide(const lsn_carrier_scan_cfg_t* cfg, const lsn_carrier_metric_t* metric, uint32_t n, uint32_t* accepted_out, uint32_t cap)
{
  return lsn::guarded([&]() -> int {
    lsn::ScanPlan sp;
    const int r = sp.init(cfg);
    if (r != LSN_SUCCESS) return r;
    if ((n && !metric) || (cap && !accepted_out)) return LSN_ERROR_INVALID_INPUTS;
    const std::vector<uint32_t> acc = lsn::scan_decide(sp.cfg, metric, n);
    for (size_t i = 0; i < acc.size() && i < cap; i++) accepted_out[i] = acc[i];
    return (int)acc.size();
  });
}

int lsn_carrier_scan(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_carrier_scan_cfg_t* cfg, lsn_carrier_t* carriers_out, uint32_t cap,
                     lsn_carrier_metric_t* metric_out)
{
  return lsn::guarded([&]() -> int { return lsn::carrier_scan(device, in, in_on_device != 0, n_in, cfg, carriers_out, cap, metric_out); });
}

int lsn_file_carrier_scan(int device, const char* path, const lsn_file_cfg_t* fc, const lsn_carrier_scan_cfg_t* ucfg, lsn_carrier_t* carriers_out, uint32_t cap,
                          lsn_carrier_metric_t* metric_out)
{
  return lsn::guarded([&]() -> int {
    if (!path || !fc || !ucfg || ucfg->struct_size != sizeof(lsn_carrier_scan_cfg_t) || fc->offset_time_samples < 0) return LSN_ERROR_INVALID_INPUTS;
    lsn_carrier_scan_cfg_t cfg = *ucfg;
    cfg.nof_antennas = fc->nof_antennas;
    cfg.sample_format = fc->sample_format;
    cfg.sample_scale = fc->sample_scale;
    lsn::ScanPlan sp;
    const int r = sp.init(&cfg);
    if (r != LSN_SUCCESS) return r;
    const LsnSampleFormat sfm = lsn_sample_format(cfg.sample_format, cfg.sample_scale);
    if (!sfm.valid || cfg.nof_antennas < 1 || cfg.nof_antennas > 8 || (cfg.antenna != LSN_SCAN_ALL_ANTENNAS && cfg.antenna >= cfg.nof_antennas) || (cap && !carriers_out))
      return LSN_ERROR_INVALID_INPUTS;
    const size_t smp = (size_t)sfm.bytes * cfg.nof_antennas, total = (size_t)sp.n_in * smp;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return LSN_ERROR_INVALID_INPUTS;
    struct Fd { int fd; ~Fd() { close(fd); } } guard{fd};
    std::vector<uint8_t> head(total);
    const uint64_t off0 = (uint64_t)fc->offset_time_samples * smp;
    size_t o = 0;
    while (o < total) {
      const ssize_t k = pread(fd, head.data() + o, total - o, (off_t)(off0 + o));
      if (k < 0) throw std::runtime_error("carrier scan: read failed");
      if (k == 0) return LSN_ERROR_INVALID_INPUTS;   // the file is shorter than the head the scan reads
      o += (size_t)k;
    }
    return lsn::carrier_scan(device, head.data(), false, sp.n_in, &cfg, carriers_out, cap, metric_out);
  });
}

int lsn_carrier_channel(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_carrier_channel_cfg_t* cfg, float* out, int out_on_device, uint64_t n_out)
{
  return lsn::guarded([&]() -> int { return lsn::carrier_channel(device, in, in_on_device != 0, n_in, cfg, out, out_on_device != 0, n_out); });
}

int lsn_carrier_channel_span(const lsn_carrier_channel_cfg_t* cfg, uint64_t n_out, uint64_t in_end, lsn_resample_span_t* out)
{
  return lsn::guarded([&]() -> int {
    lsn::ResamplePlan plan;
    const int r = lsn::channel_plan(cfg, plan);
    if (r != LSN_SUCCESS || !out) return r != LSN_SUCCESS ? r : LSN_ERROR_INVALID_INPUTS;
    if (n_out >= (1ull << 40)) return LSN_ERROR_INVALID_INPUTS;
    std::memset(out, 0, sizeof *out);
    out->taps = plan.taps;
    plan.inputSpan(cfg->out_first, n_out, out->in_lo, out->in_hi);
    const uint64_t inside = plan.outputsInside(in_end);
    out->max_out = inside > cfg->out_first ? inside - cfg->out_first : 0;
    return LSN_SUCCESS;
  });
}

}  // extern "C"

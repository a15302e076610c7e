// lsn_clock.cc - the sample clock of a recording, measured ahead of the replay from the positions of its PSS occurrences:
// the plan of the windows (coarse to fine) and the line fit are host work in double and touch no GPU, like lsn_resample_span; the correlation
// over the windows is k_pss_track of stage_sync.hip; argmax and the parabola through the peak on the host.  The answer is an input of
// lsn_phy_process_file_rate - nothing in the engine, k_ofdm or the file source knows about it.  tests/clock_model.py is written from the definition
// in include/ltesniffer_amd.h, not from this file.  Product code: no CPU fallback for the correlation, nothing from oracle/ is included or linked.
#include "lsn_hip.h"
#include "../kernels/lsn_dev.h"
#include "lsn_clock.h"
#include "lsn_rates.h"
#include "lsn_resample_launch.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

void lsn_launch_pss_track(const cf32* x, const void* tab, uint32_t nper, uint32_t max_lag, const cf32* p, uint32_t N, float* C, hipStream_t s);

namespace lsn {
namespace {

struct TrackSlice {  // LsnTrackSlice of stage_sync.hip
  uint64_t off;
  uint32_t nlag, c_off;
};

struct ClockGeom {
  uint32_t N, W5, Q;
};

inline uint32_t half0(uint32_t q, uint32_t W5, double max_ppm) { return kClockGuard + (uint32_t)std::ceil((double)q * (double)W5 * max_ppm * 1e-6); }

// N, W5 and Q (the periods whose round-0-style window lies inside the samples) of a configuration, or the refusal; need_q = false (one round on windows
// the caller names): fewer than four periods are no refusal
int clock_geometry(const lsn_clock_cfg_t* cfg, uint64_t nof_samples, ClockGeom& g, bool need_q = true)
{
  if (!cfg || cfg->struct_size != sizeof(lsn_clock_cfg_t)) return LSN_ERROR_INVALID_INPUTS;
  g.N = symbol_size(cfg->nof_prb, cfg->rates);
  if (!g.N || cfg->n_id_2 > 2 || !(cfg->max_ppm > 0.0 && cfg->max_ppm <= 1000.0) || !std::isfinite(cfg->cfo_hz)) return LSN_ERROR_INVALID_INPUTS;
  if (cfg->pss_pos >= (1ull << 40) || nof_samples >= (1ull << 40)) return LSN_ERROR_INVALID_INPUTS;
  g.W5 = 75 * g.N;
  const uint32_t maxp = cfg->max_periods && cfg->max_periods < kClockMaxPeriods ? cfg->max_periods : kClockMaxPeriods;
  g.Q = 0;
  for (uint32_t q = 0; q < maxp; q++) {
    const uint64_t c = cfg->pss_pos + (uint64_t)q * g.W5, h = half0(q, g.W5, cfg->max_ppm);
    if (c < h || c + h + g.N > nof_samples) break;
    g.Q++;
  }
  return g.Q >= 4 || !need_q ? LSN_SUCCESS : LSN_ERROR_INVALID_INPUTS;
}

int clock_plan(const lsn_clock_cfg_t* cfg, uint64_t nof_samples, uint32_t round, const lsn_clock_t* prev, lsn_clock_obs_t* w, uint32_t cap)
{
  ClockGeom g;
  const int r = clock_geometry(cfg, nof_samples, g);
  if (r != LSN_SUCCESS) return r;
  uint32_t qprev = 0, qr = std::min(g.Q, kClockRound0);
  for (uint32_t i = 0; i < round; i++) {
    if (qr == g.Q) return 0;  // the round in front of this one covered every period
    qprev = qr;
    qr = std::min(g.Q, 4 * qr);
  }
  if (round && (!prev || !prev->found || !(std::fabs(prev->eps) < 0.01) || !(std::fabs(prev->pss_pos0) < 0x1p40))) return LSN_ERROR_INVALID_INPUTS;
  if (!w) return (int)qr;
  if (cap < qr) return LSN_ERROR_INVALID_INPUTS;
  for (uint32_t q = 0; q < qr; q++) {
    lsn_clock_obs_t& o = w[q];
    std::memset(&o, 0, sizeof o);
    o.period = q;
    if (!round) {
      o.centre = (int64_t)(cfg->pss_pos + (uint64_t)q * g.W5);
      o.half_width = half0(q, g.W5, cfg->max_ppm);
    } else {
      const uint32_t d = qprev - 1;  // the previous fit may be one sample off across its span
      o.centre = (int64_t)std::floor(prev->pss_pos0 + ((double)q * (double)g.W5) * (1.0 + prev->eps) + 0.5);
      o.half_width = kClockGuard + (q + d - 1) / d;
    }
  }
  return (int)qr;
}

int clock_fit(const lsn_clock_obs_t* obs, uint32_t n, uint32_t W5, lsn_clock_t* out)
{
  if (!out) return LSN_ERROR_INVALID_INPUTS;
  std::memset(out, 0, sizeof *out);
  if (!obs || !n || !W5) return LSN_ERROR_INVALID_INPUTS;
  out->nof_periods = n;
  std::vector<uint32_t> keep;
  std::vector<double> peaks;
  for (uint32_t i = 0; i < n; i++)
    if (obs[i].valid) { keep.push_back(i); peaks.push_back((double)obs[i].peak); }
  if (keep.empty()) return 0;
  std::sort(peaks.begin(), peaks.end());
  const size_t m = peaks.size();
  const double thr = 0.25 * (m & 1 ? peaks[m / 2] : 0.5 * (peaks[m / 2 - 1] + peaks[m / 2]));
  {
    std::vector<uint32_t> k2;
    for (uint32_t i : keep) if ((double)obs[i].peak >= thr) k2.push_back(i);
    keep.swap(k2);
  }
  // the line is fitted to d = pos - q W5 (exact in a double: pos is an integer plus a fraction, q W5 an integer), so the numbers stay small
  auto dq = [&](uint32_t i) { return obs[i].pos - (double)obs[i].period * (double)W5; };
  double slope = 0.0, icpt = 0.0;
  auto ols = [&](const std::vector<uint32_t>& k) {
    double qm = 0.0, dm = 0.0;
    for (uint32_t i : k) { qm += (double)obs[i].period; dm += dq(i); }
    qm /= (double)k.size();
    dm /= (double)k.size();
    double sqq = 0.0, sqd = 0.0;
    for (uint32_t i : k) { const double a = (double)obs[i].period - qm; sqq += a * a; sqd += a * (dq(i) - dm); }
    if (!(sqq > 0.0)) return false;
    slope = sqd / sqq;
    icpt = dm - slope * qm;
    return true;
  };
  auto resid = [&](uint32_t i) { return dq(i) - (icpt + slope * (double)obs[i].period); };
  out->nof_used = (uint32_t)keep.size();
  if (keep.size() < 2 || !ols(keep)) return 0;
  {
    std::vector<uint32_t> k2;
    for (uint32_t i : keep) if (!(std::fabs(resid(i)) > 1.0)) k2.push_back(i);
    keep.swap(k2);
  }
  out->nof_used = (uint32_t)keep.size();
  if (keep.size() < 2 || !ols(keep)) return 0;
  double ss = 0.0, mx = 0.0;
  for (uint32_t i : keep) { const double e = resid(i); ss += e * e; mx = std::max(mx, std::fabs(e)); }
  out->rms_residual = std::sqrt(ss / (double)keep.size());
  out->max_residual = mx;
  out->eps = slope / (double)W5;
  out->pss_pos0 = icpt;
  out->found = keep.size() >= 4 && 2 * keep.size() >= (size_t)n && out->rms_residual <= 0.5 ? 1u : 0u;
  return (int)out->found;
}

void clock_replica(const lsn_clock_cfg_t& cfg, uint32_t N, cf32* out)
{
  std::vector<double> pd(2 * (size_t)N);
  pss_replica_d(cfg.n_id_2, N, (double)cfg.cfo_hz, pd.data());
  for (uint32_t k = 0; k < N; k++) out[k] = {(float)pd[2 * k], (float)pd[2 * k + 1]};
}

// pos / peak / valid of one window from its C values
void observe(const float* C, lsn_clock_obs_t& o)
{
  const uint32_t L = 2 * o.half_width + 1;
  uint32_t b = 0;
  for (uint32_t i = 1; i < L; i++) if (C[i] > C[b]) b = i;
  o.valid = 0;
  o.pos = 0.0;
  o.peak = C[b];
  if (b == 0 || b + 1 >= L) return;
  const double cm = (double)C[b - 1], c0 = (double)C[b], cp = (double)C[b + 1], den = cm - 2.0 * c0 + cp;
  if (!(den < 0.0)) return;
  o.pos = (double)(o.centre - (int64_t)o.half_width + (int64_t)b) + 0.5 * (cm - cp) / den;
  o.valid = 1;
}

// lags and place in C of every window; each must lie inside the samples
int slices_of(const lsn_clock_obs_t* w, uint32_t n, uint32_t N, uint64_t nof_samples, std::vector<TrackSlice>& tab, uint32_t& total, uint32_t& max_lag)
{
  if (!w || !n || n > 65535) return LSN_ERROR_INVALID_INPUTS;
  tab.resize(n);
  uint64_t tot = 0;
  max_lag = 0;
  for (uint32_t i = 0; i < n; i++) {
    const int64_t h = (int64_t)w[i].half_width;
    if (h > (1 << 22) || w[i].centre < h || w[i].centre > ((int64_t)1 << 40) || (uint64_t)(w[i].centre + h) + N > nof_samples) return LSN_ERROR_INVALID_INPUTS;
    tab[i].off = (uint64_t)(w[i].centre - h);
    tab[i].nlag = (uint32_t)(2 * h + 1);
    tab[i].c_off = (uint32_t)tot;
    tot += tab[i].nlag;
    max_lag = std::max(max_lag, tab[i].nlag);
  }
  if (tot > (1u << 30)) return LSN_ERROR_INVALID_INPUTS;
  total = (uint32_t)tot;
  return LSN_SUCCESS;
}

// device, stream and the replica of one estimate; correlate() is one launch of k_pss_track
struct Tracker {
  const uint32_t N;
  hipStream_t st = nullptr;
  DevBuf bp;
  cf32* d_p = nullptr;

  explicit Tracker(uint32_t n) : N(n) {}
  ~Tracker() { if (st) (void)hipStreamDestroy(st); }

  int open(int device, const lsn_clock_cfg_t& cfg)
  {
    if (!have_device(device)) return LSN_ERROR_NO_DEVICE;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    std::vector<cf32> rep(N);
    clock_replica(cfg, N, rep.data());
    d_p = bp.alloc<cf32>(N);
    HIP_CHECK(hipMemcpyAsync(d_p, rep.data(), N * sizeof(cf32), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return LSN_SUCCESS;
  }

  // tab[i].off counts samples of d_x; work queued on st in front of this call is waited for
  void correlate(const cf32* d_x, const std::vector<TrackSlice>& tab, uint32_t total, uint32_t max_lag, std::vector<float>& C)
  {
    DevBuf bt, bc;
    TrackSlice* d_t = bt.alloc<TrackSlice>(tab.size());
    float* d_c = bc.alloc<float>(total);
    HIP_CHECK(hipMemcpyAsync(d_t, tab.data(), tab.size() * sizeof(TrackSlice), hipMemcpyHostToDevice, st));
    lsn_launch_pss_track(d_x, d_t, (uint32_t)tab.size(), max_lag, d_p, N, d_c, st);
    C.resize(total);
    HIP_CHECK(hipMemcpyAsync(C.data(), d_c, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }

  // the slices packed one behind the other in host memory (tab[i].off already counts samples of `packed`)
  void correlatePacked(const std::vector<cf32>& packed, const std::vector<TrackSlice>& tab, uint32_t total, uint32_t max_lag, std::vector<float>& C)
  {
    DevBuf bx;
    cf32* d_x = bx.alloc<cf32>(packed.size());
    HIP_CHECK(hipMemcpyAsync(d_x, packed.data(), packed.size() * sizeof(cf32), hipMemcpyHostToDevice, st));
    correlate(d_x, tab, total, max_lag, C);
  }
};

void observe_all(const std::vector<float>& C, const std::vector<TrackSlice>& tab, lsn_clock_obs_t* w, float* corr_out)
{
  for (size_t i = 0; i < tab.size(); i++) observe(C.data() + tab[i].c_off, w[i]);
  if (corr_out) std::memcpy(corr_out, C.data(), C.size() * sizeof(float));
}

// one round on samples in memory: device memory is read in place, of host memory only the slices cross the link
int track_memory(Tracker& T, const cf32* iq, bool on_device, uint64_t nof_samples, lsn_clock_obs_t* w, uint32_t n, float* corr_out)
{
  std::vector<TrackSlice> tab;
  uint32_t total = 0, max_lag = 0;
  const int r = slices_of(w, n, T.N, nof_samples, tab, total, max_lag);
  if (r != LSN_SUCCESS) return r;
  std::vector<float> C;
  if (on_device) {
    T.correlate(iq, tab, total, max_lag, C);
  } else {
    std::vector<cf32> packed((size_t)total + (size_t)n * (T.N - 1));
    size_t o = 0;
    for (auto& s : tab) {
      const size_t len = (size_t)s.nlag + T.N - 1;
      std::memcpy(packed.data() + o, iq + s.off, len * sizeof(cf32));
      s.off = o;
      o += len;
    }
    T.correlatePacked(packed, tab, total, max_lag, C);
  }
  observe_all(C, tab, w, corr_out);
  return LSN_SUCCESS;
}

// the rounds: plan, track, fit, until the round that covers every period.  track(windows, n) fills the observations or returns < 0
template <class TrackFn>
int estimate_rounds(const lsn_clock_cfg_t* cfg, uint64_t nof_samples, const ClockGeom& g, TrackFn&& track, lsn_clock_t* out, lsn_clock_obs_t* obs_out)
{
  std::vector<lsn_clock_obs_t> w(g.Q);
  lsn_clock_t prev, cur;
  std::memset(&prev, 0, sizeof prev);
  std::memset(&cur, 0, sizeof cur);
  uint32_t nobs = 0;
  for (uint32_t r = 0;; r++) {
    const int n = clock_plan(cfg, nof_samples, r, r ? &prev : nullptr, w.data(), g.Q);
    if (n < 0) return n;
    if (n == 0) break;
    bool inside = true;
    for (int i = 0; i < n; i++) {
      const int64_t h = (int64_t)w[i].half_width;
      if (w[i].centre < h || (uint64_t)(w[i].centre + h) + g.N > nof_samples) inside = false;
    }
    if (!inside) {  // a fit that places a window outside the samples is no fit
      cur.found = 0;
      cur.nof_rounds = r + 1;
      break;
    }
    const int rc = track(w.data(), (uint32_t)n);
    if (rc < 0) return rc;
    nobs = (uint32_t)n;
    clock_fit(w.data(), nobs, g.W5, &cur);
    cur.nof_rounds = r + 1;
    if (!cur.found) break;
    prev = cur;
    if (nobs == g.Q) break;
  }
  *out = cur;
  if (cur.found) {
    const uint64_t d = (cfg->pss_pos + (uint64_t)g.W5 - cfg->sf_start % g.W5) % g.W5;  // PSS behind the subframe start, nominal samples
    out->sample_rate_hz = 15000.0 * (double)g.N * (1.0 + cur.eps);
    double s = cur.pss_pos0 - (double)d * (1.0 + cur.eps);
    while (s < 0.0) s += (double)g.W5 * (1.0 + cur.eps);
    out->sf_start = s;
  }
  if (obs_out && nobs) std::memcpy(obs_out, w.data(), (size_t)nobs * sizeof(lsn_clock_obs_t));
  return cur.found ? 1 : 0;
}

// antenna `ant` of the interleaved file, samples [lo, lo + cnt) -> dst, in the file's format
struct ClockFile {
  int fd = -1;
  uint64_t samples = 0;  // per antenna
  uint32_t nant = 1, ant = 0, bytes = 8;
  ~ClockFile() { if (fd >= 0) close(fd); }
  int open(const char* path)
  {
    fd = ::open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) return LSN_ERROR_INVALID_INPUTS;
    samples = (uint64_t)sb.st_size / ((uint64_t)bytes * nant);
    return LSN_SUCCESS;
  }
  void read(uint64_t lo, uint64_t cnt, uint8_t* dst, std::vector<uint8_t>& tmp) const
  {
    const size_t spb = (size_t)bytes * nant, total = (size_t)cnt * spb;
    uint8_t* buf = nant == 1 ? dst : (tmp.resize(total), tmp.data());
    size_t o = 0;
    while (o < total) {
      const ssize_t k = pread(fd, buf + o, total - o, (off_t)(lo * spb + o));
      if (k <= 0) throw std::runtime_error("clock estimate: read failed");
      o += (size_t)k;
    }
    if (nant != 1)
      for (uint64_t i = 0; i < cnt; i++) std::memcpy(dst + i * bytes, buf + i * spb + (size_t)ant * bytes, bytes);
  }
};

// file samples of one antenna -> cf32 by the file source's rule
void to_cf32(const uint8_t* raw, uint32_t fmt, float scale, size_t cnt, cf32* out)
{
  if (fmt == LSN_FMT_CF32) { std::memcpy(out, raw, cnt * sizeof(cf32)); return; }
  for (size_t i = 0; i < cnt; i++) {
    if (fmt == LSN_FMT_SC16) {
      int16_t q[2];
      std::memcpy(q, raw + 4 * i, 4);
      out[i] = {(float)q[0] * scale, (float)q[1] * scale};
    } else {
      const int8_t* q = (const int8_t*)raw + 2 * i;
      out[i] = {(float)q[0] * scale, (float)q[1] * scale};
    }
  }
}

}  // namespace
}  // namespace lsn

extern "C" {

int lsn_clock_plan(const lsn_clock_cfg_t* cfg, uint64_t nof_samples, uint32_t round, const lsn_clock_t* previous, lsn_clock_obs_t* windows, uint32_t cap)
{
  return lsn::guarded([&]() -> int { return lsn::clock_plan(cfg, nof_samples, round, previous, windows, cap); });
}

int lsn_clock_fit(const lsn_clock_obs_t* obs, uint32_t n, uint32_t W5, lsn_clock_t* out)
{
  return lsn::guarded([&]() -> int { return lsn::clock_fit(obs, n, W5, out); });
}

int lsn_clock_replica(const lsn_clock_cfg_t* cfg, float* out)
{
  return lsn::guarded([&]() -> int {
    lsn::ClockGeom g;
    if (!cfg || cfg->struct_size != sizeof(lsn_clock_cfg_t) || !out) return LSN_ERROR_INVALID_INPUTS;
    g.N = lsn::symbol_size(cfg->nof_prb, cfg->rates);
    if (!g.N || cfg->n_id_2 > 2 || !std::isfinite(cfg->cfo_hz)) return LSN_ERROR_INVALID_INPUTS;
    lsn::clock_replica(*cfg, g.N, (cf32*)out);
    return LSN_SUCCESS;
  });
}

int lsn_clock_track(int device, const void* iq, int iq_on_device, uint64_t nof_samples, const lsn_clock_cfg_t* cfg, lsn_clock_obs_t* windows, uint32_t n,
                    float* corr_out)
{
  return lsn::guarded([&]() -> int {
    lsn::ClockGeom g;
    const int r = lsn::clock_geometry(cfg, nof_samples, g, false);
    if (r != LSN_SUCCESS) return r;
    if (!iq) return LSN_ERROR_INVALID_INPUTS;
    std::vector<lsn::TrackSlice> tab;
    uint32_t total = 0, max_lag = 0;
    const int rs = lsn::slices_of(windows, n, g.N, nof_samples, tab, total, max_lag);  // refused before a device is touched
    if (rs != LSN_SUCCESS) return rs;
    lsn::Tracker T(g.N);
    const int ro = T.open(device, *cfg);
    if (ro != LSN_SUCCESS) return ro;
    return lsn::track_memory(T, (const cf32*)iq, iq_on_device != 0, nof_samples, windows, n, corr_out);
  });
}

int lsn_clock_estimate(int device, const void* iq, int iq_on_device, uint64_t nof_samples, const lsn_clock_cfg_t* cfg, lsn_clock_t* out, lsn_clock_obs_t* obs_out,
                       uint32_t cap)
{
  return lsn::guarded([&]() -> int {
    if (out) std::memset(out, 0, sizeof *out);
    lsn::ClockGeom g;
    const int r = lsn::clock_geometry(cfg, nof_samples, g);
    if (r != LSN_SUCCESS) return r;
    if (!iq || !out || (obs_out && cap < g.Q)) return LSN_ERROR_INVALID_INPUTS;
    lsn::Tracker T(g.N);
    const int ro = T.open(device, *cfg);
    if (ro != LSN_SUCCESS) return ro;
    return lsn::estimate_rounds(cfg, nof_samples, g, [&](lsn_clock_obs_t* w, uint32_t n) {
      return lsn::track_memory(T, (const cf32*)iq, iq_on_device != 0, nof_samples, w, n, nullptr);
    }, out, obs_out);
  });
}

int lsn_file_clock_estimate(int device, const char* path, const lsn_file_cfg_t* fc, const lsn_file_rate_t* rate, uint32_t antenna, const lsn_clock_cfg_t* cfg,
                            lsn_clock_t* out)
{
  using namespace lsn;
  return guarded([&]() -> int {
    if (out) std::memset(out, 0, sizeof *out);
    if (!path || !fc || !out || !cfg || cfg->struct_size != sizeof(lsn_clock_cfg_t)) return LSN_ERROR_INVALID_INPUTS;
    const LsnSampleFormat sfm = lsn_sample_format(fc->sample_format, fc->sample_scale);
    if (!sfm.valid || fc->nof_antennas < 1 || fc->nof_antennas > 8 || antenna >= fc->nof_antennas || fc->offset_time_samples < 0) return LSN_ERROR_INVALID_INPUTS;
    const uint32_t N = symbol_size(cfg->nof_prb, cfg->rates);
    if (!N) return LSN_ERROR_INVALID_INPUTS;
    const double fs = 15000.0 * (double)N;
    const uint64_t offset = (uint64_t)fc->offset_time_samples;
    ResamplePlan plan;
    double frac = 0.0;
    if (rate) {  // the sizes lsn_phy_process_file_rate knows
      if (rate->struct_size != offsetof(lsn_file_rate_t, center_offset_hz) && rate->struct_size != sizeof(lsn_file_rate_t)) return LSN_ERROR_INVALID_INPUTS;
      const double center = rate->struct_size == sizeof(lsn_file_rate_t) ? rate->center_offset_hz : 0.0;
      if (!(rate->offset_time_frac >= 0.0 && rate->offset_time_frac < 4.0e18)) return LSN_ERROR_INVALID_INPUTS;
      frac = rate->offset_time_frac;
      const double whole = std::floor(frac);
      const int rp = plan.init(rate->sample_rate_hz, fs, 15000.0 * (6.0 * (double)cfg->nof_prb + 1.0), offset + (uint64_t)whole, frac - whole, center);
      if (rp != LSN_SUCCESS) return rp;
    }
    ClockFile f;
    f.nant = fc->nof_antennas;
    f.ant = antenna;
    f.bytes = sfm.bytes;
    const int rf = f.open(path);
    if (rf != LSN_SUCCESS) return rf;
    const uint64_t nof_samples = rate ? plan.outputsInside(f.samples) : (f.samples > offset ? f.samples - offset : 0);
    ClockGeom g;
    const int r = clock_geometry(cfg, nof_samples, g);
    if (r != LSN_SUCCESS) return r;
    Tracker T(g.N);
    const int ro = T.open(device, *cfg);
    if (ro != LSN_SUCCESS) return ro;
    ResampleTables tb;
    if (rate) {
      tb.upload(plan, T.st);
      HIP_CHECK(hipStreamSynchronize(T.st));
    }
    std::vector<uint8_t> tmp, raw;
    const int found = estimate_rounds(cfg, nof_samples, g, [&](lsn_clock_obs_t* w, uint32_t n) -> int {
      std::vector<TrackSlice> tab;
      uint32_t total = 0, max_lag = 0;
      const int rs = slices_of(w, n, g.N, nof_samples, tab, total, max_lag);
      if (rs != LSN_SUCCESS) return rs;
      const size_t packed_len = (size_t)total + (size_t)n * (g.N - 1);
      std::vector<float> C;
      if (!rate) {
        std::vector<cf32> packed(packed_len);
        size_t o = 0;
        for (auto& s : tab) {
          const size_t len = (size_t)s.nlag + g.N - 1;
          raw.resize(len * sfm.bytes);
          f.read(offset + s.off, len, raw.data(), tmp);
          to_cf32(raw.data(), fc->sample_format, sfm.scale, len, packed.data() + o);
          s.off = o;
          o += len;
        }
        T.correlatePacked(packed, tab, total, max_lag, C);
      } else {
        // the input span of every slice, one antenna, in the file's format, one behind the other (each on an 8-byte boundary); k_resample turns each into its slice
        struct In { int64_t lo; uint64_t len; size_t at; };
        std::vector<In> in(n);
        size_t bytes = 0;
        for (uint32_t i = 0; i < n; i++) {
          int64_t lo, hi;
          plan.inputSpan(tab[i].off, (uint64_t)tab[i].nlag + g.N - 1, lo, hi);
          lo = std::max<int64_t>(lo, 0);
          hi = std::min<int64_t>(hi, (int64_t)f.samples);
          in[i] = {lo, hi > lo ? (uint64_t)(hi - lo) : 0, bytes};
          bytes += ((size_t)in[i].len * sfm.bytes + 7) & ~(size_t)7;
        }
        raw.resize(bytes);
        for (uint32_t i = 0; i < n; i++) f.read((uint64_t)in[i].lo, in[i].len, raw.data() + in[i].at, tmp);
        DevBuf br, bx;
        uint8_t* d_raw = br.alloc<uint8_t>(bytes);
        cf32* d_x = bx.alloc<cf32>(packed_len);
        HIP_CHECK(hipMemcpyAsync(d_raw, raw.data(), bytes, hipMemcpyHostToDevice, T.st));
        size_t o = 0;
        for (uint32_t i = 0; i < n; i++) {
          const uint64_t len = (uint64_t)tab[i].nlag + g.N - 1;
          lsn_launch_resample({d_raw + in[i].at, fc->sample_format, sfm.scale, in[i].lo, in[i].len, 1, 0}, plan.cell(tab[i].off, (uint32_t)len, tb, d_x + o, len), T.st);
          tab[i].off = o;
          o += len;
        }
        T.correlate(d_x, tab, total, max_lag, C);
      }
      observe_all(C, tab, w, nullptr);
      return LSN_SUCCESS;
    }, out, nullptr);
    if (found == 1) {  // in samples of the file, from its first one
      if (rate) {
        out->sample_rate_hz = rate->sample_rate_hz * (1.0 + out->eps);
        out->sf_start = (double)offset + frac + out->sf_start * (rate->sample_rate_hz / fs);
      } else {
        out->sf_start += (double)offset;
      }
    }
    return found;
  });
}

}  // extern "C"

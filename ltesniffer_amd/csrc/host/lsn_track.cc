// lsn_track.cc - the timing loop of a pushed stream (lsn_track.h).  HIP-free host arithmetic, as lsn_stream.cc: it runs - and is tested
// (tests/test_track_model.py, written from the definition in include/ltesniffer_amd.h, not from this file) - on a machine with no GPU.  The unit is compiled with
// -ffp-contract=off like the rest of the library: every double expression below is one rounding per operation, in the order written.
#include "../../../include/ltesniffer_amd.h"
#include "lsn_track.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace lsn {

int track_cfg_resolve(double kp, double ki, double max_ppm, uint32_t lost_after, TrackCfg& out)
{
  TrackCfg c;
  if (kp != 0.0) c.kp = kp;
  if (ki != 0.0) c.ki = ki;
  if (max_ppm != 0.0) c.max_ppm = max_ppm;
  if (lost_after) c.lost_after = lost_after;
  if (!std::isfinite(c.kp) || !std::isfinite(c.ki) || !(c.kp > 0.0) || !(c.ki > 0.0) || !(c.max_ppm > 0.0 && c.max_ppm <= 120.0)) return LSN_ERROR_INVALID_INPUTS;
  out = c;
  return LSN_SUCCESS;
}

__int128 track_delta(double rate_in, double rate_out, uint32_t seglen, double c)
{
  const double scale = std::ldexp(rate_in / rate_out, 64);
  const double v = scale * c;
  return (__int128)std::nearbyint(v / (double)seglen);
}

__int128 track_step(const TrackCfg& cfg, double rate_in, double rate_out, uint32_t seglen, TrackLoop& s, double e, bool valid)
{
  const double lim = cfg.max_ppm * 1e-6 * (double)seglen;
  auto clamp = [lim](double v) { return v > lim ? lim : (v < -lim ? -lim : v); };
  if (valid) {
    const double ie = cfg.ki * e, pe = cfg.kp * e;
    const double in = clamp(s.integ + ie);
    const double u = pe + in;
    // anti-windup: while the correction sits at its limit and e pushes it further out, the integrator keeps its value - the error a limited correction cannot
    // remove yet must not be integrated, or it comes back as overshoot once the limit lets go
    if (!((u > lim && e > 0.0) || (u < -lim && e < 0.0))) s.integ = in;
    s.corr = clamp(pe + s.integ);
    s.invalid_run = 0;
    s.lost = 0;
  } else {
    s.corr = s.integ;
    if (s.invalid_run < 0xFFFFFFFFu) s.invalid_run++;
    if (s.invalid_run >= cfg.lost_after) s.lost = 1;
  }
  return track_delta(rate_in, rate_out, seglen, s.corr);
}

bool track_observe(const float* C, uint32_t d, double& e, double& peak)
{
  uint32_t b = 0;
  for (uint32_t j = 1; j < kTrackLags; j++) if (C[j] > C[b]) b = j;
  e = 0.0;
  peak = (double)C[b];
  if (b == 0 || b + 1 >= kTrackLags) return false;
  const double cm = (double)C[b - 1], c0 = (double)C[b], cp = (double)C[b + 1], den = (cm - 2.0 * c0) + cp;
  if (!(den < 0.0)) return false;
  const double frac = 0.5 * (cm - cp) / den;
  e = (((double)b - 6.0) + frac) * (double)d;
  return true;
}

bool TrackPeaks::accept(double peak)
{
  if (n) {
    double sum = 0.0;
    for (uint32_t i = 0; i < n; i++) sum = sum + hist[(at + 8 - n + i) % 8];   // oldest first
    if (!(peak >= 0.25 * (sum / (double)n))) return false;
  }
  hist[at] = peak;
  at = (at + 1) % 8;
  if (n < 8) n++;
  return true;
}

u128 track_widened_step(u128 step, double max_ppm)
{
  // step (1 + max_ppm 1e-6), rounded up: the product of the top 64 bits of a step below 2^67 with a factor in 2^-32 units is exact enough and errs upwards
  const uint64_t f = (uint64_t)std::ceil(max_ppm * 1e-6 * 4294967296.0) + 1;   // units of 2^-32
  return step + (((step >> 32) + 1) * f);
}

void TrackCell::init(const ResamplePlan* plan, uint32_t sflen_, uint32_t N_, uint32_t tti0, uint64_t max_sf, double r_in, const TrackCfg& c, bool enable, double initial_ppm)
{
  rs = plan; sflen = sflen_; N = N_; max_subframes = max_sf; rate_in = r_in; rate_out = 15000.0 * (double)N_; cfg = c; enabled = enable;
  start_tti = tti0;
  const uint32_t ph = tti0 % kTrackSegSubframes;
  first_nsf = ph ? kTrackSegSubframes - ph : kTrackSegSubframes;
  first_has_pss = ph == 0;
  loop = TrackLoop();
  if (enabled) loop.integ = loop.corr = initial_ppm * 1e-6 * (double)(kTrackSegSubframes * sflen);
  peaks = TrackPeaks();
  entered = false; h = 0; nq = 0; nvalid = ninvalid = 0; last_e = 0.0;
}

void TrackCell::enter()
{
  const uint32_t seglen = kTrackSegSubframes * sflen;
  const u128 b = endBase();
  const uint64_t s0 = segEnd();
  __int128 delta;
  if (needsMeasurement()) {
    if (!nq) throw std::runtime_error("track: a segment entered before its measurement came back");
    const Meas m = q[0];
    const Attempt at = fq[0];
    q[0] = q[1];
    fq[0] = fq[1];
    nq--;
    if (at.due) frameTakeIn(h - 1, at);   // (frame sync) the attempt of segment h - 1, two in front of the one that begins here: in front of a jump's restart
    delta = enabled ? track_step(cfg, rate_in, rate_out, seglen, loop, m.e, m.valid) : 0;
  } else {
    delta = enabled ? track_delta(rate_in, rate_out, seglen, loop.corr) : 0;   // segments 0 and 1: the opened rate times 1 + initial_ppm 1e-6
  }
  u128 b2 = b;
  if (searchResultDue()) {   // behind the loop's step: an accepted search moves the position once, by o outputs at the step of the segment that was searched
    if (!search.done) throw std::runtime_error("track: a segment entered before its search came back");
    if (search.accepted) {
      const __int128 jump = (__int128)search.offset * (__int128)search.step;
      b2 = (u128)((__int128)b + jump);
      loop.invalid_run = 0;
      acq_jumps += jump;
      acq_jump_segment = h + 1;
      if (fs.on) { fs.active = true; fs.g = h + 1; fs.checks++; }   // (frame sync) the check of this jump, a running one restarted
    }
    search = Search();
  }
  h = entered ? h + 1 : 0;
  entered = true;
  sf0 = s0;
  nsf = h ? kTrackSegSubframes : first_nsf;
  if (max_subframes && sf0 + nsf > max_subframes) nsf = sf0 < max_subframes ? (uint32_t)(max_subframes - sf0) : 0;
  base = b2;
  step = (u128)((__int128)rs->step + delta);
  span = rs->spanAt(step);   // ResamplePlan::init's rule at this segment's step; the run length and the lanes per output stay the plan's
  if (span < rs->span) span = rs->span;
  if (acq && enabled && !search.active && loop.invalid_run >= acq_after) {   // a search of this segment is due
    search.active = true; search.h = h; search.base = base; search.step = step; search.span = span;
  }
}

// the attempt of segment a, looked at on entering segment a + 2 (enter(): h is still a + 1): a result nobody waits for - no check runs, or the segment lies in
// front of the running check's first - is dropped
void TrackCell::frameTakeIn(uint64_t a, const Attempt& at)
{
  if (!fs.active || a < fs.g) return;
  int32_t delta = 0;
  const uint32_t counted = (uint32_t)((start_tti + segmentStart(a) + fs.shift) % kTtiWrap);
  if (at.launched && track_frame_decide(at.mib, fs.nof_prb, fs.nof_ports, counted, delta)) {
    fs.last_sfn = at.mib.sfn; fs.last_delta = delta; fs.accept_segment = a;
    if (delta) {
      fs.shift = (uint32_t)(((int64_t)fs.shift + kTtiWrap + delta) % kTtiWrap);
      fs.relabelled++;
      fs.relabel_segment = a + kTrackDelay;
    } else {
      fs.confirmed++;
    }
    fs.active = false;
  } else if (a - fs.g + 1 >= fs.tries) {
    fs.given_up++;
    fs.active = false;
  }
}

void TrackCell::searchInputSpan(int64_t& lo, int64_t& hi) const
{
  const int64_t half = (int64_t)rs->taps / 2;
  const u128 last = search.base + (u128)((uint64_t)kAcqSpanSubframes * sflen - 1) * search.step;
  lo = (int64_t)(uint64_t)(search.base >> 64) - half + 1;
  hi = (int64_t)(uint64_t)(last >> 64) + half + 1;
}

void TrackCell::searched(const float* C)
{
  if (!search.active || search.done) throw std::runtime_error("track: a search result nobody waits for");
  search.done = true;
  if (C) {
    const uint32_t d = track_lag_spacing(N);
    search.accepted = track_acquire_decide(C, kTrackSegSubframes * sflen / d, d, N, acq_min_ratio, search.hist_mean, search.offset, acq_peak, acq_ratio);
    acq_offset = search.offset;
  }
  if (search.accepted) acq_accepted++; else acq_rejected++;
}

bool track_acquire_decide(const float* C, uint32_t n, uint32_t d, uint32_t N, double min_ratio, double history_mean, int64_t& offset, double& peak, double& ratio)
{
  uint32_t b = 0;
  for (uint32_t i = 1; i < n; i++) if (C[i] > C[b]) b = i;
  double far = 0.0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t fw = i >= b ? i - b : i + n - b, dist = std::min(fw, n - fw);
    if (dist > kAcqFar && (double)C[i] > far) far = (double)C[i];
  }
  peak = (double)C[b];
  ratio = far > 0.0 ? peak / far : (peak > 0.0 ? INFINITY : 0.0);
  const int64_t W5 = 75 * (int64_t)N, p = (int64_t)track_pss_index(N);
  offset = (((int64_t)b * d - p + W5 / 2) % W5 + W5) % W5 - W5 / 2;
  return peak > 0.0 && peak >= min_ratio * far && !(history_mean >= 0.0 && !(peak >= 0.25 * history_mean));
}

bool mib_parse(const LsnCand cand[4], lsn_mib_t& out)
{
  static const uint32_t bw[6] = {6, 15, 25, 50, 75, 100};
  static const uint32_t ng6[4] = {1, 3, 6, 12};
  std::memset(&out, 0, sizeof(out));
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t mask = cand[q].rnti & 0xFFFFu;
    const uint32_t ports = mask == 0x0000u ? 1u : (mask == 0xFFFFu ? 2u : (mask == 0x5555u ? 4u : 0u));
    const uint32_t mib = (uint32_t)(cand[q].bits >> 40);  // 24 bits, first bit = MSB
    if (!ports || !mib) continue;  // an all-zero block passes the CRC trivially
    const uint32_t bwi = mib >> 21;
    if (bwi > 5) continue;
    out.found = 1; out.sfn_offset = q; out.nof_ports = ports; out.mib_bits = mib;
    out.nof_prb = bw[bwi]; out.phich_length = (mib >> 20) & 1u; out.phich_resources_x6 = ng6[(mib >> 18) & 3u];
    out.sfn = ((((mib >> 10) & 0xFFu) << 2) + q) % 1024u;
    return true;
  }
  return false;
}

bool track_frame_decide(const lsn_mib_t& mib, uint32_t nof_prb, uint32_t nof_ports, uint32_t counted_tti, int32_t& delta)
{
  delta = 0;
  if (!mib.found || mib.nof_prb != nof_prb || mib.nof_ports != nof_ports) return false;
  if (counted_tti % kTrackSegSubframes) throw std::runtime_error("frame sync: a segment that does not begin on a TTI multiple of 5");
  const uint32_t t = 10u * (mib.sfn % 1024u);
  const uint32_t m = (t + kTtiWrap - counted_tti % kTtiWrap) % kTtiWrap;
  delta = m > kTtiWrap / 2 ? (int32_t)m - (int32_t)kTtiWrap : (int32_t)m;
  return true;
}

uint64_t track_acquire_keep(u128 step, double max_ppm, uint32_t sflen)
{
  return (uint64_t)(((u128)((uint64_t)kAcqKeepSubframes * sflen) * track_widened_step(step, max_ppm)) >> 64) + 1;
}

void TrackCell::measured(const float* C, const Attempt* at)
{
  Meas m = {false, 0.0};
  if (C && enabled) {
    double e, peak;
    if (track_observe(C, track_lag_spacing(N), e, peak) && peaks.accept(peak)) { m.valid = true; m.e = e; last_e = e; }
  }
  if (search.active && nvalid + ninvalid == search.h + 1) {   // this is the measurement of segment h + 1 (every segment has one, in order): the history the decision reads
    search.hist_mean = -1.0;
    if (peaks.n) {
      double sum = 0.0;
      for (uint32_t i = 0; i < peaks.n; i++) sum = sum + peaks.hist[(peaks.at + 8 - peaks.n + i) % 8];
      search.hist_mean = sum / (double)peaks.n;
    }
  }
  if (m.valid) nvalid++; else ninvalid++;
  if (nq >= kTrackDelay) throw std::runtime_error("track: more measurements than the loop's delay");
  fq[nq] = at ? *at : Attempt();
  q[nq++] = m;
}

uint64_t TrackCell::completeInSegment(uint64_t pushed) const
{
  if (!entered || !nsf) return segEnd();
  const uint64_t half = rs->taps / 2;
  if (pushed <= half) return sf0;
  const u128 lim = (u128)(pushed - half) << 64;   // positions below lim read no sample at or behind `pushed` (ResamplePlan::outputsInside)
  if (base >= lim) return sf0;
  const u128 n = (lim - 1 - base) / step + 1;
  const u128 sf = n / sflen;
  return sf0 + (sf >= nsf ? nsf : (uint64_t)sf);
}

void TrackCell::inputSpan(uint64_t sf_lo, uint64_t sf_hi, int64_t& lo, int64_t& hi) const
{
  const int64_t half = (int64_t)rs->taps / 2;
  const u128 first = position(sf_lo), last = sf_hi > sf_lo ? position(sf_hi) - step : first;
  lo = (int64_t)(uint64_t)(first >> 64) - half + 1;
  hi = (int64_t)(uint64_t)(last >> 64) + half + 1;
}

double TrackCell::positionDrift(uint64_t next_sf) const
{
  const u128 real = position(next_sf), nominal = rs->position(next_sf * sflen);
  const __int128 diff = (__int128)(real - nominal);
  return std::ldexp((double)diff, -64);
}

}  // namespace lsn

extern "C" {

static int track_cfg_of(const lsn_stream_track_cfg_t* cfg, lsn::TrackCfg& out)
{
  if (!cfg || cfg->struct_size != sizeof(lsn_stream_track_cfg_t)) return LSN_ERROR_INVALID_INPUTS;
  return lsn::track_cfg_resolve(cfg->kp, cfg->ki, cfg->max_ppm, cfg->lost_after, out);
}

int lsn_stream_track_step(const lsn_stream_track_cfg_t* cfg, double rate_in_hz, double rate_out_hz, uint32_t seglen, lsn_stream_track_state_t* state, double e, int valid,
                          uint64_t* delta_hi, uint64_t* delta_lo)
{
  lsn::TrackCfg c;
  const int r = track_cfg_of(cfg, c);
  if (r != LSN_SUCCESS) return r;
  if (!state || !delta_hi || !delta_lo || !seglen || !(rate_in_hz > 0.0) || !(rate_out_hz > 0.0) || !std::isfinite(rate_in_hz / rate_out_hz) || !std::isfinite(e)) return LSN_ERROR_INVALID_INPUTS;
  lsn::TrackLoop s;
  s.integ = state->integrator; s.corr = state->correction; s.invalid_run = state->invalid_run; s.lost = state->lost;
  const __int128 d = lsn::track_step(c, rate_in_hz, rate_out_hz, seglen, s, e, valid != 0);
  state->integrator = s.integ; state->correction = s.corr; state->invalid_run = s.invalid_run; state->lost = s.lost;
  *delta_hi = (uint64_t)((unsigned __int128)d >> 64);
  *delta_lo = (uint64_t)(unsigned __int128)d;
  return LSN_SUCCESS;
}

int lsn_pss_timing_error(const float* C, uint32_t d, double* e, double* peak)
{
  if (!C || !d || !e || !peak) return LSN_ERROR_INVALID_INPUTS;
  return lsn::track_observe(C, d, *e, *peak) ? 1 : 0;
}

int lsn_frame_sync_decide(const lsn_mib_t* mib, uint32_t nof_prb, uint32_t nof_ports, uint32_t counted_tti, int32_t* delta)
{
  if (!mib || !delta || counted_tti >= lsn::kTtiWrap || (mib->found && mib->sfn >= 1024u)) return LSN_ERROR_INVALID_INPUTS;
  try {
    return lsn::track_frame_decide(*mib, nof_prb, nof_ports, counted_tti, *delta) ? 1 : 0;
  } catch (const std::exception&) {
    return LSN_ERROR;
  }
}

int lsn_pss_acquire_decide(const float* C, uint32_t n, uint32_t d, uint32_t N, double min_ratio, double history_mean, int64_t* offset, double* peak, double* ratio)
{
  if (!C || !offset || !peak || !ratio || N < 128 || N > 2048 || d != lsn::track_lag_spacing(N) || (uint64_t)n * d != 75ull * N || std::isnan(history_mean)) return LSN_ERROR_INVALID_INPUTS;
  if (min_ratio == 0.0) min_ratio = lsn::kAcqMinRatio;
  if (!std::isfinite(min_ratio) || min_ratio < 1.0) return LSN_ERROR_INVALID_INPUTS;
  return lsn::track_acquire_decide(C, n, d, N, min_ratio, history_mean, *offset, *peak, *ratio) ? 1 : 0;
}

}  // extern "C"

// lsn_track.h - the timing loop of a pushed stream (lsn_stream_track): the segments that make a cell's resampler position piecewise linear
// in the output index, the observation taken from the 13 values of k_pss_timing, and the proportional-integral loop that turns it into the step of a later segment.
// Plain host arithmetic in doubles and 128-bit integers, no HIP header (like lsn_stream.h): it runs - and is tested (tests/test_track_model.py) - on a machine with
// no GPU.  Every decision here is a function of (input samples, configuration) only; nothing depends on when a push arrived.
#pragma once
#include "../../../include/ltesniffer_amd.h"
#include "lsn_resample.h"
#include "lsn_types.h"

namespace lsn {

static constexpr uint32_t kTrackLags = 13;        // l_j = (j - 6) d
static constexpr uint32_t kTrackSegSubframes = 5; // one half frame: a PSS in the first subframe of every segment behind the first
static constexpr uint32_t kTrackDelay = 2;        // the measurement of segment h decides the step of segment h + 2
// re-acquisition
static constexpr uint32_t kAcqSpanSubframes = 6;  // a search reads segment h and one subframe more, all at segment h's step
static constexpr uint32_t kAcqDelay = 3;          // and is taken in on entering segment h + 3
static constexpr uint32_t kAcqFar = 8;            // lags around the maximum that do not count as another peak
static constexpr uint32_t kAcqKeepSubframes = 8;  // 6 for the span of the segment behind, 2.5 for a backward jump, rounded up
static constexpr double kAcqMinRatio = 3.0;       // the geometric mean of the ratio measured on noise (1.86) and with the cell present (5.1)
// frame sync
static constexpr uint32_t kFrameTries = 8;        // attempts of one check: four radio frames, one PBCH period
static constexpr uint32_t kFrameMaxTries = 64;
static constexpr uint32_t kTtiWrap = 10240;

inline uint32_t track_lag_spacing(uint32_t N) { return N / 128 ? N / 128 : 1; }
// index, inside a subframe 0 / 5, of the first useful sample of the PSS symbol: symbol 6 of slot 0 with the normal prefix, symbol 5 with the extended one - 13 N / 2
// either way (160 + 6 144 = 1024 = 2048 / 2 at N = 2048; 6 512 / 4 + 5 at the extended prefix)
inline uint32_t track_pss_index(uint32_t N) { return 13 * N / 2; }

struct TrackCfg {   // defaults resolved
  double kp = 0.25, ki = 1.0 / 32.0, max_ppm = 100.0;
  uint32_t lost_after = 40;
};

struct TrackLoop {
  double integ = 0.0;   // I, output samples per segment
  double corr = 0.0;    // c, output samples to recover per segment: what the step in force was formed from
  uint32_t invalid_run = 0, lost = 0;
};

// one step of the loop, in this order of operations (the unit is compiled without fused contraction):
//   valid:   I' = clamp(I + Ki e); I = I' unless Kp e + I' lies beyond the limit on the side e pushes to; c = clamp(Kp e + I)          invalid:  c = I
//   clamp to +- lim = max_ppm 1e-6 seglen;  delta = (int128) nearbyint(ldexp(rate_in / rate_out, 64) * c / seglen)
// -> delta: step = step_nom + delta
__int128 track_step(const TrackCfg& cfg, double rate_in, double rate_out, uint32_t seglen, TrackLoop& s, double e, bool valid);
// the step delta of a correction c alone (the loop's last line)
__int128 track_delta(double rate_in, double rate_out, uint32_t seglen, double c);

// the observation of one window: j* = first maximum; geometrically valid when 0 < j* < 12 and the parabola through the three values opens downwards;
// e = (j* - 6 + 0.5 (C[j*-1] - C[j*+1]) / (C[j*-1] - 2 C[j*] + C[j*+1])) d, peak = C[j*]
bool track_observe(const float* C, uint32_t d, double& e, double& peak);

// peak >= 0.25 mean(the last up to 8 valid peaks); the first one is valid.  A valid peak joins the history
struct TrackPeaks {
  double hist[8] = {};
  uint32_t n = 0, at = 0;
  bool accept(double peak);
};

// One cell's segments.  Segment h holds output subframes [sf0_h, sf0_h + n_h); position(m) = base_h + (m - sf0_h sflen) step_h, base_(h+1) = base_h + n_h sflen step_h.
// Only the segment that holds the next subframe to resample is kept: a segment is entered when the one in front of it is complete, with the measurement of the
// segment two in front of it (enter()).
struct TrackCell {
  const ResamplePlan* rs = nullptr;
  uint32_t sflen = 0, N = 0;
  uint64_t max_subframes = 0;
  double rate_in = 0.0, rate_out = 0.0;
  bool enabled = false;
  uint32_t first_nsf = kTrackSegSubframes;   // subframes of segment 0: up to the first TTI that is a multiple of 5
  bool first_has_pss = true;
  TrackCfg cfg;
  TrackLoop loop;
  TrackPeaks peaks;
  // the current segment
  uint64_t h = 0;            // its index; valid once entered
  bool entered = false;
  uint64_t sf0 = 0; uint32_t nsf = 0;
  u128 base = 0, step = 0;
  uint32_t span = 0;         // samples one run of the kernel stages at this step
  // measurements: those of segments h - 2 and h - 1 wait in q[] until their turn
  struct Meas { bool valid; double e; };
  Meas q[kTrackDelay] = {};
  uint32_t nq = 0;
  uint64_t nvalid = 0, ninvalid = 0;
  double last_e = 0.0;
  // re-acquisition (off unless reacquire() was called): at most one search per cell is in flight.  It is due on entering segment h, after the loop's step, when
  // invalid_run >= after; its span is segment h's base and step; its result - searched() - is taken in by the enter() of segment h + 3
  struct Search {
    bool active = false, launched = false, done = false, accepted = false;
    uint64_t h = 0;
    u128 base = 0, step = 0;
    uint32_t span = 0;
    double hist_mean = -1.0;   // the valid-peak history behind the measurement of segment h + 1 (measured() fills it; < 0: empty)
    int64_t offset = 0;
  };
  bool acq = false;
  uint32_t acq_after = 0;
  double acq_min_ratio = kAcqMinRatio;
  Search search;
  uint64_t acq_launched = 0, acq_accepted = 0, acq_rejected = 0, acq_jump_segment = 0;
  double acq_peak = 0.0, acq_ratio = 0.0;
  int64_t acq_offset = 0;
  __int128 acq_jumps = 0;    // the sum of all jumps, 2^-64 input samples

  // frame sync (off unless frameSync() was called): an accepted jump starts a check at the segment it takes force at, g.  Every segment
  // a = g .. g + tries - 1 of a running check is due an attempt - a PBCH decode of its first subframe -, whose result comes in with the segment's measurement
  // (measured()) and waits with it: enter() looks at the result of segment a when it enters segment a + 2 and at no other time, so nothing depends on when a
  // status call fetched it.  Accepted: the shift changes, from this segment on; `tries` results without one: given up.  Either ends the check
  struct Attempt { bool due = false, launched = false; lsn_mib_t mib = {}; };   // due: the segment was one of a running check when its first piece was launched
  struct Frame {
    bool on = false, hold = true;
    uint32_t tries = kFrameTries, nof_prb = 0, nof_ports = 0;
    bool active = false;
    uint64_t g = 0;
    uint32_t shift = 0;        // subframes, mod 10240: the TTI of subframe sf is start_tti + sf + shift
    uint64_t checks = 0, attempts = 0, confirmed = 0, relabelled = 0, given_up = 0, accept_segment = 0, relabel_segment = 0, held = 0;
    uint32_t last_sfn = 0;
    int32_t last_delta = 0;
  };
  Frame fs;
  Attempt fq[kTrackDelay] = {};   // in step with q[]
  uint32_t start_tti = 0;
  void frameSync(uint32_t tries, bool hold, uint32_t nof_prb, uint32_t nof_ports) { fs.on = true; fs.tries = tries ? tries : kFrameTries; fs.hold = hold; fs.nof_prb = nof_prb; fs.nof_ports = nof_ports; }
  bool frameAttemptDue() const { return fs.active && entered && h >= fs.g && h - fs.g < fs.tries; }   // of the current segment
  bool frameHolding() const { return fs.active && fs.hold; }                                           // the current segment's subframes are not submitted
  uint32_t tti(uint64_t sf) const { return (uint32_t)((start_tti + sf + fs.shift) % kTtiWrap); }     // of a subframe of the current segment
  uint64_t segmentStart(uint64_t a) const { return a ? first_nsf + (a - 1) * kTrackSegSubframes : 0; }  // the first subframe of segment a

  void reacquire(uint32_t after, double min_ratio) { acq = true; acq_after = after ? after : cfg.lost_after; acq_min_ratio = min_ratio != 0.0 ? min_ratio : kAcqMinRatio; }
  bool searchResultDue() const { return search.active && entered && h + 1 == search.h + kAcqDelay; }   // the next enter() takes the search's result in
  void searchInputSpan(int64_t& lo, int64_t& hi) const;   // input samples the search in flight reads
  // the result: C the values of k_pss_acquire (75 N / d of them), null = the search could not be launched (its span reads a gap) - rejected
  void searched(const float* C);

  void init(const ResamplePlan* plan, uint32_t sflen_, uint32_t N_, uint32_t start_tti, uint64_t max_sf, double r_in, const TrackCfg& c, bool enable, double initial_ppm);
  uint64_t segEnd() const { return entered ? sf0 + nsf : 0; }       // first subframe behind the current segment (0 before segment 0 is entered)
  bool hasPss() const { return h ? true : first_has_pss; }
  u128 endBase() const { return entered ? base + (u128)nsf * sflen * step : rs->start; }
  u128 position(uint64_t sf) const { return entered ? base + (u128)(sf - sf0) * sflen * step : rs->start; }   // sf inside the current segment, or its end
  // the next segment begins at subframe segEnd().  needs(): it takes a measurement out of q first (segments 2 ...)
  bool needsMeasurement() const { return entered && h + 1 >= kTrackDelay; }
  void enter();
  void frameTakeIn(uint64_t a, const Attempt& at);
  // the measurement of the current segment, taken from its first subframe: C null = none could be taken (no PSS, a gap, the cell not enabled)
  // at: the attempt of that segment, if it was due one (frame sync; null: none)
  void measured(const float* C, const Attempt* at = nullptr);
  // subframes [.., n) of the cell that are complete once `pushed` samples have arrived, counted up to the end of the current segment
  uint64_t completeInSegment(uint64_t pushed) const;
  void inputSpan(uint64_t sf_lo, uint64_t sf_hi, int64_t& lo, int64_t& hi) const;   // subframes [sf_lo, sf_hi) of the current segment
  double positionDrift(uint64_t next_sf) const;   // real minus nominal position of the first output of subframe next_sf, input samples
};

// LSN_SUCCESS and the resolved configuration, or LSN_ERROR_INVALID_INPUTS: gains not finite or not positive, max_ppm outside (0, 120]
int track_cfg_resolve(double kp, double ki, double max_ppm, uint32_t lost_after, TrackCfg& out);
// the plan's step widened by 1 + max_ppm 1e-6, rounded up: the fastest a tracked cell moves through the ring
u128 track_widened_step(u128 step, double max_ppm);

// ---- re-acquisition (lsn_stream_reacquire) ----
// the decision over the values of k_pss_acquire, C[n] with n d = 75 N: i* the first maximum, peak = C[i*], far the largest value whose circular distance from i*
// is above kAcqFar lags; accepted when peak > 0, peak >= min_ratio far and peak >= 0.25 history_mean (history_mean < 0: an empty history accepts);
// offset = ((i* d - 13 N / 2 + 75 N / 2) mod 75 N) - 75 N / 2 output samples: the nearest PSS; ratio = peak / far (far = 0: infinity, or 0 when peak is 0 too)
bool track_acquire_decide(const float* C, uint32_t n, uint32_t d, uint32_t N, double min_ratio, double history_mean, int64_t& offset, double& peak, double& ratio);
// input samples a cell with re-acquisition keeps behind what it keeps anyway: kAcqKeepSubframes output subframes at the widened step
uint64_t track_acquire_keep(u128 step, double max_ppm, uint32_t sflen);

// ---- frame sync (lsn_stream_frame_sync) ----
// the four candidates of k_pbch_viterbi (radio-frame phases 0 .. 3: bits, CRC mask) -> the MIB of the first one that passes; true when one did.  lsn_phy_mib_decode's
// host part: out is zeroed first
bool mib_parse(const LsnCand cand[4], lsn_mib_t& out);
// the decision over one attempt.  Accepted (true) when the MIB is found and its nof_prb and nof_ports are the Phy's; T = 10 sfn, C = counted_tti (below 10240: the
// TTI the attempt's subframe was counted as), delta = (T - C) mod 10240, signed in (-5120, 5120].  An accepted MIB with C mod 5 != 0 - and with it delta mod 5
// != 0 - is an internal error (throws): segments begin on TTI multiples of 5 and stay there, delta being one.
// Chance of accepting garbage: 3 CRC masks x 4 phases / 2^16, times 1/3 for the port mask, times 1/8 for the bandwidth field: about 8e-6 per attempt
bool track_frame_decide(const lsn_mib_t& mib, uint32_t nof_prb, uint32_t nof_ports, uint32_t counted_tti, int32_t& delta);

}  // namespace lsn

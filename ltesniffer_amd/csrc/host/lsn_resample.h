// lsn_resample.h - host side of the polyphase resampler (kernels/resample.hip; launchers: lsn_resample_launch.h): the plan of one rate pair - step, start, taps, bank, and the
// tuning word and NCO tables of the mixer in front of the filter - the 64.64 position arithmetic in 128-bit integers, and the launch record of a cell, which
// ResamplePlan::cell alone forms.  Definition: DESIGN.md section 3.1b.
#pragma once
#include <cstdint>
#include <vector>

// no HIP header: the plan is plain host arithmetic, and lsn_cells.cc, which builds on it, stays HIP-free.  What needs the runtime's types - the kernel launchers and
// the owner of a cell's device tables - is declared in lsn_resample_launch.h.
struct cf32;

#define LSN_RS_MAP_MAX_OUT 2u   // LSN_MAP_MAX_OUT of the public header (lsn_front_launch.cc asserts it)

// what one cell brings to a launch of its own (the launch's other arguments - raw buffer, format, scale, antennas - are the recording's: LsnFrontSource)
struct LsnResampleCell {
  uint64_t base_hi, base_lo;   // position of the cell's output 0 in this launch
  uint64_t d_lo; uint32_t d_hi;
  uint32_t taps, span;
  uint32_t sflen, sf_off;
  const float* bank;
  uint64_t w; const cf32* nco; // nco null: the cell is not translated
  const cf32* rot;
  cf32* out;
  uint64_t n_out;              // 0: the cell takes no part in this launch
  uint32_t grp, run;           // grp = 0: the run of 512 outputs, one lane per output (ratios up to 4); else the wide-ratio run: grp lanes share an output,
                               // a workgroup makes `run` outputs
  // the antenna map.  map_nout = 0: none - every antenna of the source to the row of its own number, tuned by w.  Else the cell writes map_nout rows,
  // row a cut from antenna map_src[a] of the source with tuning word map_w[a] (0: not mixed); w is unread, nco is set when a word is non-zero
  uint32_t map_nout;
  uint32_t map_src[LSN_RS_MAP_MAX_OUT];
  uint64_t map_w[LSN_RS_MAP_MAX_OUT];
};

namespace lsn {

typedef unsigned __int128 u128;

// a cell's device tables as a launch record names them; ResampleTables (lsn_resample_launch.h) owns them
struct ResampleTablePtrs {
  float* d_bank = nullptr;      // the bank ...
  const cf32* d_nco = nullptr;  // ... and, behind it in the same allocation, the mixer's tables when the plan has a tuning word
  cf32* d_rot = nullptr;        // the optional -o rotation of the outputs, [sflen]
};

struct ResamplePlan {
  u128 step = 0;       // D = round(rate_in / rate_out * 2^64)
  u128 start = 0;      // P0: position of output sample 0
  uint32_t taps = 0;   // T (even)
  uint32_t span = 0;   // input samples one run of the kernel stages
  // the run geometry, fixed by the plan's nominal step alone: grp = 0 and run = 512 for ratios up to 4; above, grp lanes share one output and a
  // workgroup makes run = 4096 / grp outputs.  A tracked segment keeps both whatever its own step is
  uint32_t grp = 0, run = 512;
  std::vector<float> bank;  // [512][T][2]: H[p][j] and H[p + 1][j] - H[p][j], float32 (row 511 reaches phase 512 through its difference)
  uint64_t tune = 0;        // W = floor(center_offset_hz / rate_in * 2^64 + 1/2) mod 2^64: input sample n is rotated by exp(-2 pi j (n W mod 2^64) / 2^64)
  std::vector<float> nco;   // tune != 0: the mixer's tables, [4096] coarse then [1024] fine (re, im), lsn_nco_tables; else empty
  // the antenna map, set by initMapped: map_nout outputs, output a from input antenna map_src[a] with tuning word map_w[a]; tune is 0 then and ONE set
  // of tables serves both words (the tables do not depend on the word).  map_nout = 0: none
  uint32_t map_nout = 0;
  uint32_t map_src[LSN_RS_MAP_MAX_OUT] = {};
  uint64_t map_w[LSN_RS_MAP_MAX_OUT] = {};

  // LSN_SUCCESS, or LSN_ERROR_INVALID_INPUTS when the pair is outside what the filter meets, or the cell at center_offset_hz does not lie inside
  // the recording (accepted range)
  // max_ratio, max_taps: the largest rate_in / rate_out and Kaiser estimate of the one-lane-per-output run; the defaults are lsn_resample's and the file source's,
  // the carrier scan's narrow-band channel lifts them to 64 and 768.  A ratio above max_ratio is accepted for the wide-ratio run when it is at most
  // kWideMaxRatio, rate_in at most kWideMaxRateIn, rate_out at least kWideMinRateOut and the estimate at most kWideMaxTaps
  static constexpr double kWideMaxRatio = 32.0, kWideMaxRateIn = 122.88e6, kWideMinRateOut = 3.84e6;
  static constexpr uint32_t kWideMaxTaps = 768, kWideRounds = 16, kWideLanes = 256;
  int init(double rate_in, double rate_out, double passband_hz, uint64_t first_sample, double first_frac, double center_offset_hz, double max_ratio = 4.0,
           uint32_t max_taps = 192);
  // init with an antenna map: the plan of the pair with no offset, then per output a the acceptance rule |center_offset_hz + offset_hz[a]| + pass band <=
  // rate_in / 2 (NaN and infinity fail it) and the word of that sum.  nof_out 1 .. LSN_RS_MAP_MAX_OUT and src[a] < nof_in, or LSN_ERROR_INVALID_INPUTS
  int initMapped(double rate_in, double rate_out, double passband_hz, uint64_t first_sample, double first_frac, double center_offset_hz, uint32_t nof_in, uint32_t nof_out,
                 const uint32_t* src, const double* offset_hz);
  static uint64_t tuning(double center_offset_hz, double rate_in);   // W of one offset
  u128 position(uint64_t m) const { return start + (u128)m * step; }
  // lanes per output of the wide-ratio run at nominal step D: 0 up to ratio 4, else the smallest power of two >= D, 8 .. 32
  static uint32_t groupOf(u128 step_)
  {
    if (step_ <= ((u128)4 << 64)) return 0;
    uint32_t g = 8;
    while (g < 32 && ((u128)g << 64) < step_) g *= 2;
    return g;
  }
  static uint32_t runOf(uint32_t grp_) { return grp_ ? kWideRounds * kWideLanes / grp_ : 512u; }
  // input samples a run of this plan stages at step step_ (the plan's own, or a tracked segment's): floor(run * step_) + T + 2
  uint32_t spanAt(u128 step_) const { return (uint32_t)(((u128)run * step_) >> 64) + taps + 2; }
  // the launch record of n_out outputs from position `base` on, `step_` apart - the ONE place a position and a step are split into the kernel's words.  A tracked
  // segment passes its own base, step and span; sf_off is the phase of output 0 inside its row of sflen outputs
  LsnResampleCell cell(u128 base, u128 step_, uint32_t span_, uint32_t sflen, uint32_t sf_off, const ResampleTablePtrs& t, cf32* out, uint64_t n_out) const
  {
    LsnResampleCell k;
    k.base_hi = (uint64_t)(base >> 64); k.base_lo = (uint64_t)base; k.d_lo = (uint64_t)step_; k.d_hi = (uint32_t)(step_ >> 64);
    k.taps = taps; k.span = span_; k.sflen = sflen; k.sf_off = sf_off; k.bank = t.d_bank; k.w = tune; k.nco = t.d_nco; k.rot = t.d_rot; k.out = out; k.n_out = n_out;
    k.grp = grp; k.run = run;
    k.map_nout = map_nout;
    for (uint32_t a = 0; a < LSN_RS_MAP_MAX_OUT; a++) { k.map_src[a] = map_src[a]; k.map_w[a] = map_w[a]; }
    return k;
  }
  // outputs [m0, m0 + n_out) of this plan, output m0 at the start of a row
  LsnResampleCell cell(uint64_t m0, uint32_t sflen, const ResampleTablePtrs& t, cf32* out, uint64_t n_out) const { return cell(position(m0), step, span, sflen, 0, t, out, n_out); }
  // input samples [lo, hi) that outputs m0 .. m0 + n - 1 read (lo may be negative: zeros in front of the recording)
  void inputSpan(uint64_t m0, uint64_t n, int64_t& lo, int64_t& hi) const;
  // number of outputs m = 0, 1, ... whose taps all lie in front of input sample in_end
  uint64_t outputsInside(uint64_t in_end) const;
};

}  // namespace lsn

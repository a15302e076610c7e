// lsn_sync_all.h - the HIP-free part of the successive cell search (lsn_sync_all.cc): which lags a cancellation changes, and the rule of a round.
// Needs nothing but the public header, so tests call it without a GPU (lsn_cell_search_all_plan, lsn_cell_search_all_decide).
#pragma once
#include "../../../include/ltesniffer_amd.h"
#include <cmath>

namespace lsn {

struct CellsCfg {  // lsn_cell_search_all_cfg_t with its defaults filled in
  uint32_t P, max_cells;
  int32_t force;
  float threshold, threshold_next, sss_ratio_min, shared_pss_ratio;  // shared_pss_ratio < 0: off
};

// threshold_next = 8: measured for 8 periods, where the floor of the correlation after a cancellation is 4.7; must be raised for fewer periods
inline int cells_cfg(const lsn_cell_search_all_cfg_t* c, CellsCfg& o)
{
  if (!c) return LSN_ERROR_INVALID_INPUTS;
  if (!std::isfinite(c->threshold) || !std::isfinite(c->threshold_next) || !std::isfinite(c->sss_ratio_min) || !std::isfinite(c->shared_pss_ratio))
    return LSN_ERROR_INVALID_INPUTS;
  if (c->nof_periods > 16 || c->max_cells > LSN_SEARCH_MAX_CELLS || c->force_n_id_2 > 2 || c->force_n_id_2 < -1 || c->threshold_next < 0.0f || c->sss_ratio_min < 0.0f)
    return LSN_ERROR_INVALID_INPUTS;
  o.P = c->nof_periods ? c->nof_periods : 8;
  o.max_cells = c->max_cells ? c->max_cells : LSN_SEARCH_MAX_CELLS;
  o.force = c->force_n_id_2;
  o.threshold = c->threshold;
  o.threshold_next = c->threshold_next != 0.0f ? c->threshold_next : 8.0f;
  o.sss_ratio_min = c->sss_ratio_min != 0.0f ? c->sss_ratio_min : 1.5f;
  o.shared_pss_ratio = c->shared_pss_ratio != 0.0f ? c->shared_pss_ratio : 0.6f;
  return LSN_SUCCESS;
}

// A cancellation writes the samples bn + j W5 + [0, N) of every occurrence j.  Lag n of period q reads q W5 + n + [0, N): it meets occurrence q when
// |n - bn| < N and occurrence q + 1 when n > bn + W5 - N - the same set modulo W5.  2 N - 1 lags from bn - (N - 1) on.
inline int cells_plan(uint32_t bn, uint32_t N, uint32_t W5, lsn_cell_search_all_plan_t* o)
{
  if (!o || !N || W5 < 2 * N || bn >= W5) return LSN_ERROR_INVALID_INPUTS;
  o->n_lag = 2 * N - 1;
  o->n_lo = bn >= N - 1 ? bn - (N - 1) : bn + W5 - (N - 1);
  o->run_lo[0] = o->n_lo;
  o->run_lo[1] = 0;
  if (o->n_lo + o->n_lag <= W5) {
    o->nof_runs = 1;
    o->run_len[0] = o->n_lag;
    o->run_len[1] = 0;
  } else {
    o->nof_runs = 2;
    o->run_len[0] = W5 - o->n_lo;
    o->run_len[1] = o->n_lag - o->run_len[0];
  }
  return LSN_SUCCESS;
}

inline int cells_decide(const CellsCfg& c, uint32_t round, float peak, double sum, uint32_t W5, const float* acc /* [2][336] */, lsn_cell_search_all_decision_t* o)
{
  if (!acc || !o || !W5) return LSN_ERROR_INVALID_INPUTS;
  *o = lsn_cell_search_all_decision_t{};
  const double mean = sum / (double)W5;
  o->p2avg = mean > 0.0 ? (float)((double)peak / mean) : 0.0f;
  float win = -1.0f;
  for (uint32_t cp = 0; cp < 2; cp++) {
    const float* a = acc + cp * 336;
    float m1 = -1.0f, m2 = -1.0f;
    uint32_t b1 = 0, b2 = 0;
    for (uint32_t h = 0; h < 336; h++) {  // lsn_cell_search's walk: first maximum, second largest
      const float v = a[h];
      if (v > m1) { m2 = m1; b2 = b1; m1 = v; b1 = h; }
      else if (v > m2) { m2 = v; b2 = h; }
    }
    if (!(m1 > win)) continue;  // normal CP on a tie
    win = m1;
    o->cp = cp;
    o->best = b1; o->second = b2;
    o->best_power = m1; o->second_power = m2;
    float mr = -1.0f;
    uint32_t br = 0;
    for (uint32_t h = 0; h < 336; h++)  // not the same N_id_1 in the other half frame: that is the best cell's own SSS seen half a frame off
      if ((h >> 1) != (b1 >> 1) && a[h] > mr) { mr = a[h]; br = h; }
    o->runner_up = br;
    o->runner_up_power = mr;
  }
  o->sss_ratio = o->second_power > 0.0f ? o->best_power / o->second_power : 0.0f;
  o->accept = round == 0 ? (o->p2avg >= c.threshold ? 1u : 0u) : (o->p2avg >= c.threshold_next && o->sss_ratio >= c.sss_ratio_min ? 1u : 0u);
  o->shared = c.shared_pss_ratio >= 0.0f && o->runner_up_power >= c.shared_pss_ratio * o->best_power && o->best_power > 0.0f ? 1u : 0u;
  return LSN_SUCCESS;
}

}  // namespace lsn

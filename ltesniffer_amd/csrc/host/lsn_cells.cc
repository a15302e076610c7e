// lsn_cells.cc - the plan of a multi-cell file replay (lsn_cells.h).  HIP-free host arithmetic: every number the reader and the kernel
// launch of a block need is formed here from the cells' ResamplePlans, so it runs - and is tested (tests/test_cells_plan.py) - on a machine with no GPU.
#include "../../../include/ltesniffer_amd.h"
#include "lsn_cells.h"
#include <algorithm>
#include <cmath>

static_assert(lsn::kFileMaxCells == LSN_FILE_MAX_CELLS, "lsn_cells.h speaks the public header's limit");

namespace lsn {

int file_rate_plan(double sample_rate_hz, uint32_t N, uint32_t nof_prb, int64_t offset_time_samples, double offset_time_frac, double center_offset_hz, ResamplePlan& plan)
{
  if (offset_time_samples < 0 || !(offset_time_frac >= 0.0 && offset_time_frac < 4.0e18)) return LSN_ERROR_INVALID_INPUTS;
  const double whole = std::floor(offset_time_frac);
  const uint64_t first = (uint64_t)offset_time_samples + (uint64_t)whole;
  return plan.init(sample_rate_hz, 15000.0 * (double)N, 15000.0 * (6.0 * (double)nof_prb + 1.0), first, offset_time_frac - whole, center_offset_hz);
}

int file_rate_plan_map(double sample_rate_hz, uint32_t N, uint32_t nof_prb, int64_t offset_time_samples, double offset_time_frac, double center_offset_hz, uint32_t nof_in,
                       uint32_t nof_out, const uint32_t* src, const double* offset_hz, ResamplePlan& plan)
{
  if (offset_time_samples < 0 || !(offset_time_frac >= 0.0 && offset_time_frac < 4.0e18)) return LSN_ERROR_INVALID_INPUTS;
  const double whole = std::floor(offset_time_frac);
  const uint64_t first = (uint64_t)offset_time_samples + (uint64_t)whole;
  return plan.initMapped(sample_rate_hz, 15000.0 * (double)N, 15000.0 * (6.0 * (double)nof_prb + 1.0), first, offset_time_frac - whole, center_offset_hz, nof_in, nof_out, src,
                         offset_hz);
}

uint64_t file_cell_total(uint64_t sf_in_file, uint64_t first_sf, uint64_t max_subframes)
{
  const uint64_t avail = sf_in_file > first_sf ? sf_in_file - first_sf : 0;
  return max_subframes ? std::min(max_subframes, avail) : avail;
}

bool file_cells_block(const FileCellPlan* cells, uint32_t n, uint32_t blk, uint64_t k, FileCellsBlock& out)
{
  out = FileCellsBlock();
  bool have = false;
  for (uint32_t c = 0; c < n && c < kFileMaxCells; c++) {
    const FileCellPlan& p = cells[c];
    const u128 before = (u128)k * blk;
    if (before >= (u128)p.total) continue;
    const uint32_t got = (uint32_t)std::min<u128>(blk, (u128)p.total - before);
    out.sf0[c] = p.first_sf + (uint64_t)before;
    out.nsf[c] = got;
    out.active++;
    if (!p.rs) continue;
    int64_t lo, hi;
    p.rs->inputSpan(out.sf0[c] * p.sflen, (uint64_t)got * p.sflen, lo, hi);
    lo -= (int64_t)p.pre; hi += (int64_t)p.pre;   // what stage 1 reads for the y1 stage 2 reads
    out.in_lo = have ? std::min(out.in_lo, lo) : lo;
    out.in_hi = have ? std::max(out.in_hi, hi) : hi;
    have = true;
  }
  out.in_lo = std::max<int64_t>(out.in_lo, 0);   // zeros in front of the recording are the kernel's
  out.in_hi = std::max(out.in_hi, out.in_lo);
  return out.active != 0;
}

uint32_t file_cells_fit(const FileCellPlan* cells, uint32_t n, uint32_t blk, uint64_t cap_samples)
{
  // the union of block 0 with every cell at b subframes, not clamped: grows with b
  auto fits = [&](uint32_t b) {
    int64_t lo = 0, hi = 0;
    for (uint32_t c = 0; c < n; c++) {
      int64_t l, h;
      cells[c].rs->inputSpan(cells[c].first_sf * cells[c].sflen, (uint64_t)b * cells[c].sflen, l, h);
      l -= (int64_t)cells[c].pre; h += (int64_t)cells[c].pre;
      lo = c ? std::min(lo, l) : l;
      hi = c ? std::max(hi, h) : h;
    }
    return (u128)(hi - lo) + 2 <= (u128)cap_samples;
  };
  if (!n || !blk || !fits(1)) return 0;
  uint32_t good = 1, bad = blk;   // fits(good); bad fits or is the first to try
  if (fits(blk)) return blk;
  while (bad - good > 1) {
    const uint32_t mid = good + (bad - good) / 2;
    if (fits(mid)) good = mid; else bad = mid;
  }
  return good;
}

}  // namespace lsn

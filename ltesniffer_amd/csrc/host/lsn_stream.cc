// lsn_stream.cc - the plan of a pushed stream (lsn_stream.h).  HIP-free host arithmetic, as lsn_cells.cc: it runs - and is tested
// (tests/test_stream_plan.py) - on a machine with no GPU.
#include "../../../include/ltesniffer_amd.h"
#include "lsn_stream.h"
#include "lsn_front_source.h"
#include <algorithm>

namespace lsn {

uint64_t stream_cell_complete(const StreamCellPlan& c, uint64_t pushed)
{
  return file_cell_total(c.rs->outputsInside(pushed > c.pre ? pushed - c.pre : 0) / c.sflen, 0, c.max_subframes);   // (ChanFilter::insideEnd)
}

uint32_t stream_cell_ready(const StreamCellPlan& c, uint64_t pushed, uint64_t done, uint32_t blk, bool flush)
{
  const uint64_t complete = stream_cell_complete(c, pushed);
  if (complete <= done) return 0;
  const uint64_t avail = complete - done;
  if (avail >= blk) return blk;
  const bool last = c.max_subframes && complete == c.max_subframes;   // nothing will follow them
  return flush || last ? (uint32_t)avail : 0;
}

int64_t stream_oldest_needed(const StreamCellPlan* cells, uint32_t n, const uint64_t* done, uint64_t pushed)
{
  int64_t oldest = (int64_t)pushed;
  for (uint32_t c = 0; c < n; c++) {
    const StreamCellPlan& p = cells[c];
    if (p.max_subframes && done[c] >= p.max_subframes) continue;   // run out
    int64_t lo, hi;
    p.rs->inputSpan(done[c] * p.sflen, p.sflen, lo, hi);
    oldest = std::min(oldest, std::max<int64_t>(lo - (int64_t)p.pre, 0));
  }
  return oldest;
}

uint64_t stream_block_input(const StreamCellPlan* cells, uint32_t n, uint32_t blk)
{
  int64_t lo = 0, hi = 0;
  for (uint32_t c = 0; c < n; c++) {
    int64_t l, h;
    cells[c].rs->inputSpan(0, (uint64_t)blk * cells[c].sflen, l, h);
    l -= (int64_t)cells[c].pre; h += (int64_t)cells[c].pre;   // what stage 1 reads for the y1 stage 2 reads
    lo = c ? std::min(lo, l) : l;
    hi = c ? std::max(hi, h) : h;
  }
  return (uint64_t)(hi - lo) + 2;
}

uint64_t stream_default_ring(const StreamCellPlan* cells, uint32_t n, uint32_t blk)
{
  const u128 want = (u128)4 * stream_block_input(cells, n, blk);
  uint64_t r = 1;
  while ((u128)r < want && r < (1ull << 32)) r <<= 1;
  return (u128)r >= want ? r : 0;
}

int stream_ring_check(const StreamCellPlan* cells, uint32_t n, uint32_t blk, uint64_t& ring_samples)
{
  if (!n || !blk) return LSN_ERROR_INVALID_INPUTS;
  if (!ring_samples) ring_samples = stream_default_ring(cells, n, blk);
  // a block of every cell between the oldest start and the newest data: a ring shorter than that is too small for the block, or the starts lie too far apart
  if (!lsn_ring_holds(ring_samples, stream_block_input(cells, n, blk))) return LSN_ERROR_INVALID_INPUTS;
  return LSN_SUCCESS;
}

}  // namespace lsn

// lsn_stream.h - the plan of a live stream that is pushed in host buffers and feeds several cells (lsn_stream_*): how many subframes of a
// cell are complete after `pushed` samples, which of them go out now, the oldest input sample any cell still needs, and the size of the ring that holds the raw
// input.  Plain host arithmetic on ResamplePlan, no HIP header (like lsn_cells.h, whose counting rules these are): a stream that received N samples in all has
// submitted, per cell, exactly the subframes a file of N samples replays.  The object that owns the device ring is lsn_stream_ring.h.
#pragma once
#include "lsn_cells.h"

namespace lsn {

struct StreamCellPlan {
  const ResamplePlan* rs = nullptr;   // formed by file_rate_plan, as every file replay's
  uint32_t sflen = 0;                 // output samples of one subframe
  uint64_t max_subframes = 0;         // 0: no end
  uint32_t pre = 0;                   // half length L of the channel filter in front of rs (FileCellPlan::pre's meaning); 0: none
};

// complete subframes of the cell once `pushed` samples have arrived: file_cell_total of the subframes whose whole input span lies in front of `pushed` (a stream
// starts at first_sf = 0).  With a filter the resampler reads y1, which `pushed` samples carry up to ChanFilter::insideEnd(pushed) = pushed - pre: the rule of
// lsn_file_cells_span
uint64_t stream_cell_complete(const StreamCellPlan& c, uint64_t pushed);
// subframes of the cell that go out in the next launch, `done` being submitted already: a whole block of blk; fewer only behind a flush, or when they are the last
// ones in front of max_subframes
uint32_t stream_cell_ready(const StreamCellPlan& c, uint64_t pushed, uint64_t done, uint32_t blk, bool flush);
// the oldest input sample any cell still needs: inputSpan's lo of subframe done[c], less pre, clamped at 0, minimised over the cells that have not run out; none
// left: pushed
int64_t stream_oldest_needed(const StreamCellPlan* cells, uint32_t n, const uint64_t* done, uint64_t pushed);
// input samples of one block of EVERY cell, from the oldest start to the newest end: the union of block 0 with all cells at blk subframes - every cell's span
// widened by pre on both sides, what its stage 1 reads - plus the two samples by
// which the floor of a position moves the ends of a later block - file_cells_fit's rule.  A ring holds the stream when it is at least this long
uint64_t stream_block_input(const StreamCellPlan* cells, uint32_t n, uint32_t blk);
// the ring the library chooses: the smallest power of two that holds four such blocks; 0: above 2^32 samples
uint64_t stream_default_ring(const StreamCellPlan* cells, uint32_t n, uint32_t blk);
// LSN_SUCCESS when a ring of ring_samples (0: the default, written back) can carry the cells: a power of two, at most 2^32, at least stream_block_input
int stream_ring_check(const StreamCellPlan* cells, uint32_t n, uint32_t blk, uint64_t& ring_samples);

}  // namespace lsn

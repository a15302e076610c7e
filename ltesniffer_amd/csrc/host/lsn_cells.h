// lsn_cells.h - the plan of a file replay that feeds several cells from one pass over the recording (lsn_file_process_cells, lsn_file_cells_span; DESIGN.md
// section 3.1e): the resampler's plan of one cell, the subframes every cell contributes to block k, and the ONE input range - the union of the cells' spans -
// that is read and copied for it.  Plain host arithmetic on ResamplePlan, no HIP header (like lsn_commit / lsn_types.h); the single-cell replay is its n = 1 case.
#pragma once
#include "lsn_resample.h"

namespace lsn {

constexpr uint32_t kFileMaxCells = 8;   // LSN_FILE_MAX_CELLS: the cells' kernel arguments travel in one argument block (k_resample_cells)

// The plan of one cell of a recording made at sample_rate_hz: rate pair sample_rate_hz -> 15000 N, pass band 15 kHz (6 nof_prb + 1), output sample 0 at input
// position offset_time_samples + offset_time_frac (the whole part of the fraction goes to the integer), tuning word of center_offset_hz.
// LSN_ERROR_INVALID_INPUTS: a negative or non-finite start, or what ResamplePlan::init refuses.
int file_rate_plan(double sample_rate_hz, uint32_t N, uint32_t nof_prb, int64_t offset_time_samples, double offset_time_frac, double center_offset_hz, ResamplePlan& plan);
// The same through an antenna map: nof_out outputs, output a cut from antenna src[a] of the recording's nof_in at center_offset_hz +
// offset_hz[a].  LSN_ERROR_INVALID_INPUTS also for a source outside the recording and an output that does not lie inside it (ResamplePlan::initMapped).
int file_rate_plan_map(double sample_rate_hz, uint32_t N, uint32_t nof_prb, int64_t offset_time_samples, double offset_time_frac, double center_offset_hz, uint32_t nof_in,
                       uint32_t nof_out, const uint32_t* src, const double* offset_hz, ResamplePlan& plan);

struct FileCellPlan {
  const ResamplePlan* rs = nullptr;   // null: the file is at the engine's rate (single-cell replay through k_file_unpack) - such a cell has counts but no span
  uint32_t sflen = 0;                 // output samples of one subframe
  uint64_t first_sf = 0;              // output subframe the replay starts with (LSN_TTI_FROM_MIB: the first whose MIB decoded)
  uint64_t total = 0;                 // subframes the cell replays: file_cell_total
  uint32_t pre = 0;                   // half length L of the channel filter in front of rs (lsn_chanfilt.h): the cell's span is L samples wider on both sides; 0: none
};
// sf_in_file output subframes lie inside the recording, the replay starts at first_sf and stops after max_subframes (0: at the end)
uint64_t file_cell_total(uint64_t sf_in_file, uint64_t first_sf, uint64_t max_subframes);

struct FileCellsBlock {
  int64_t in_lo = 0, in_hi = 0;       // input samples [in_lo, in_hi) of the block: the union of the spans of the cells that take part, clamped at sample 0
  uint32_t active = 0;                // cells with nsf > 0
  uint64_t sf0[kFileMaxCells] = {};   // first output subframe of the cell in this block ...
  uint32_t nsf[kFileMaxCells] = {};   // ... and how many (0: the cell has run out)
};
// block k = output subframes [first_sf + k blk, first_sf + (k + 1) blk) of every cell, clipped by the cell's total.  false: every cell has run out.
bool file_cells_block(const FileCellPlan* cells, uint32_t n, uint32_t blk, uint64_t k, FileCellsBlock& out);
// the largest block size <= blk whose input fits cap_samples in EVERY block: the union of block 0 with all cells at full length, plus the two samples by which the
// floor of a position can move the ends of a later block.  0: not even one subframe per cell fits - the cells' starts lie too far apart.
uint32_t file_cells_fit(const FileCellPlan* cells, uint32_t n, uint32_t blk, uint64_t cap_samples);

}  // namespace lsn

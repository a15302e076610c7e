// lsn_front_launch.h - the chain that brings a cell's samples from a raw buffer to its Phy's block buffer, in ONE copy for every ingest path (file replay:
// lsn_file.cc; pushed stream: lsn_stream_ring.cc): the optional channel filter, stage 1 (lsn_chanfilt_launch.h), into the cell's intermediate, and the polyphase
// resampler, stage 2 (lsn_resample_launch.h), out of that - or out of the raw buffer when the cell has no filter.  DESIGN.md section 3.1l.
#pragma once
#include "lsn_resample_launch.h"
#include "lsn_chanfilt_launch.h"

namespace lsn {

// what a cell brings to every launch of the chain.  The tables are freed with the struct: its owner destroys it only when the work that reads them is complete
struct FrontCell {
  ResampleTables tb;              // the plan's bank and NCO tables, the -o rotation
  ChanFirTables ft;               // the filter's taps and its mixer's tables
  const ChanFilter* cf = nullptr; // null or L == 0: no stage 1
  cf32* mid = nullptr;            // the intermediate, the cell's Phy's (Engine::chanBuffer): how large it must be and when it is reserved is the caller's business ...
  uint64_t mid_cap = 0;           // ... and the samples of all antennas it holds (Engine::chanBufferSamples)
  bool filtered() const { return cf && cf->L; }
};

// One launch of the chain for n cells out of src, queued on s.  k[c]: the resampler's record of cell c as the caller formed it (n_out = 0: the cell takes no
// part); [lo[c], hi[c]): the input span that piece reads.  All cells are filtered or none.  Filtered: ONE k_chan_fir launch (k_chan_fir_ring out of a ring) writes
// y1 over exactly chan_mid_span of each piece into its cell's intermediate, then one k_resample per cell reads that (k_resample_cells takes one source per launch);
// a span that does not fit throws "<what>'s filtered samples do not fit the intermediate buffer" in front of every launch.  Unfiltered: k_resample for one cell
// out of a linear buffer, else one k_resample_cells (k_resample_ring out of a ring) for all - the _map kernels when a cell of the launch has an antenna map
// (unfiltered cells only; src.nant is the recording's, a mapped cell's output rows are its Phy's).
void lsn_launch_front(const LsnFrontSource& src, const FrontCell* const* cells, const LsnResampleCell* k, const int64_t* lo, const int64_t* hi, uint32_t n, hipStream_t s,
                      const char* what);

}  // namespace lsn

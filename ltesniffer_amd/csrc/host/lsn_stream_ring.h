// lsn_stream_ring.h - the object behind lsn_stream_*: the raw input of a live stream in ONE device ring, the cells' Phys fed out of it by k_resample_ring
//  - or, when the cells have a channel filter, by k_chan_fir_ring and one k_resample per cell (section 3.1j).  The counting is lsn_stream.h's; this is the part that speaks to the HIP runtime and to the engines.
// A tracked stream (track(), section 3.1h) counts by the segments of lsn_track.h instead and measures every segment's PSS with k_pss_timing; with reacquire()
// (section 3.1k) it searches a cell that has lost its PSS with k_pss_acquire and keeps 8 subframes of input more per such cell; with frameSync() (section 3.1m) a jump
// is followed by PBCH decodes on the Phy's side scratch until one says which TTI the cell is at.
#pragma once
#include "lsn_engine.h"
#include "lsn_front_launch.h"
#include "lsn_stream.h"
#include "lsn_track.h"
#include <deque>
#include <memory>
#include <mutex>
#include <vector>

namespace lsn {

class StreamRing {
public:
  struct CellSpec {
    Engine* e = nullptr;
    ResamplePlan plan;            // file_rate_plan's; of a filtered cell: the plan with no centre offset (tune = 0), as in the file source
    ChanFilter filt;              // L != 0: stage 1 in front of plan (all cells or none: lsn_stream_open)
    float offset_freq_hz = 0.0f;
    uint32_t start_tti = 0, update_meta_period = 0;
    uint64_t max_subframes = 0;
  };
  // the caller (lsn_stream_open) has checked cells, block and ring: stream_ring_check passes and blk subframes fit the Phys' block buffers
  StreamRing(int device, uint32_t nant, uint32_t fmt, float sample_scale, uint32_t blk, uint64_t ring_samples, std::vector<CellSpec> cells);
  ~StreamRing();
  int setup();                                  // ring, streams, block buffers, banks, the filters' taps and intermediates: every allocation of the stream's life
  int push(const void* iq, uint64_t n);         // iq null: a gap of n zero samples
  int flush();
  // the timing loop (lsn_stream_track): accepted before the first sample only; a refusal leaves the stream as it was
  int track(const lsn_stream_track_cfg_t& cfg, double rate_in /* the stream's sample rate */);
  int trackStatus(lsn_stream_track_status_t* out);
  // re-acquisition (lsn_stream_reacquire): after track(), before the first sample; a refusal leaves the stream as it was
  int reacquire(const lsn_stream_reacquire_cfg_t& cfg);
  int reacquireStatus(lsn_stream_reacquire_status_t* out);
  // frame sync (lsn_stream_frame_sync): after reacquire(), before the first sample; a refusal leaves the stream as it was
  int frameSync(const lsn_stream_frame_sync_cfg_t& cfg);
  int frameSyncStatus(lsn_stream_frame_sync_status_t* out);
  uint64_t pushedSamples() const { return pushed; }
  uint64_t ringSamples() const { return ring_samples; }
  uint32_t blockSubframes() const { return blk; }
  size_t nofCells() const { return cells.size(); }
  uint64_t cellDone(size_t c) const { return cells[c].done; }
  int cellStatus(size_t c) const { return cells[c].rc; }
  int failedCode() const { return failed; }
  int64_t oldestNeeded() const;
  std::mutex mtx;                               // one call at a time (lsn_capi.cc takes it)

private:
  static constexpr int NSLOT_MAX = 8;
  struct Cell {
    CellSpec s;
    uint32_t sflen = 0;
    uint64_t done = 0;
    int rc = LSN_SUCCESS;
    // what the cell brings to every launch (lsn_front_launch.h): the plan's tables and the -o rotation and, of a filtered cell (front.cf = &s.filt), the filter's
    // tables and the Phy's intermediate - one serves every block-buffer slot, the launches being ordered on st_run.  The tables go with the cell, behind
    // ~StreamRing's body, which has waited for every engine and synchronised both streams
    FrontCell front;
    uint64_t launches = 0;              // block buffer of launch k: slot k mod nslot ...
    uint64_t mark[NSLOT_MAX] = {};       // ... free again when the engine has consumed the chunks up to this mark (0: never used)
    // a tracked stream (runReadyTracked): the block buffer fills segment by segment
    TrackCell tk;
    uint64_t filled = 0;                 // subframes resampled into block buffers, done <= filled <= done + blk
    cf32* d_rep = nullptr;               // the PSS replica, [N]
    float* h_C = nullptr;                // pinned, [TRACK_SLOTS][13]: k_pss_timing writes, the host reads behind the event
    // the measurement of segment h: timing false = none could be taken.  due: the segment is one of a running frame check; mib: its attempt was launched, and
    // its candidates land in h_cand's slot.  ev (null: nothing was launched) lies behind both
    struct Pending { uint64_t h; hipEvent_t ev; uint32_t slot; bool timing, due, mib; };
    std::deque<Pending> pending;
    // re-acquisition: the span of the search in flight (TrackCell::search) is resampled into acq_x and k_pss_acquire writes its values into acq_C
    cf32* acq_x = nullptr;               // [6][antenna][sflen]
    float* acq_C = nullptr;              // pinned, [75 N / d]
    hipEvent_t acq_ev = nullptr;         // behind the search that was launched
    uint64_t acq_keep = 0;               // input samples kept behind what the cell needs anyway (0: no re-acquisition)
    LsnCand* h_cand = nullptr;           // frame sync: pinned, [TRACK_SLOTS][4]: the candidates of the attempts in flight
  };
  static constexpr uint32_t TRACK_SLOTS = 4;   // at most kTrackDelay measurements of a cell are in flight
  struct Launch { hipEvent_t ev; int64_t lo; };   // recorded behind a launch that read the ring from recording sample lo on (filtered: the widened span's)
  void writeRing(const uint8_t* src, uint64_t n);
  int runReady(bool flush_all);
  int runReadyTracked(bool flush_all);
  // the steps the two loops share.  launchRing: the cells in k (n_out != 0) resampled out of the ring, cell c reading the recording samples [lo[c], hi[c]), behind
  // the copies queued so far, and the event behind it into `inflight`; `what` names the input in the refusals ("stream: a block").  The launches are
  // lsn_launch_front's over the union of the spans, each widened by its cell's L: unfiltered ONE k_resample_ring, filtered ONE k_chan_fir_ring and one k_resample per
  // cell.  bufferFor: the block buffer the cell fills next; empty (nothing of the next
  // block is in it yet): waits until the block it carried last has been through stage A.  submitBlock: the first nsf subframes of that buffer go to the cell's Phy
  void launchRing(const LsnResampleCell* k, const int64_t* lo, const int64_t* hi, const char* what);
  bool filtered() const { return cells[0].s.filt.L != 0; }
  // y1 samples the largest resampler piece of one launch reads at `step`: blk subframes, plus the two samples by which the floor of a position moves the ends
  uint64_t midSamples(const Cell& c, u128 step) const;
  int reserveMid(Cell& c, uint64_t samples);
  uint64_t insideEnd(const Cell& c) const { return c.s.filt.insideEnd(pushed); }   // what of y1 the samples pushed so far carry (L = 0: pushed)
  cf32* bufferFor(Cell& q, bool empty = true);
  void submitBlock(Cell& q, uint32_t nsf);   // (a tracked cell: at the TTI its TrackCell counts; while a frame check holds the cell the subframes are dropped instead)
  void closeBlock(Cell& q, uint32_t nsf, bool held, uint32_t tti);   // submitBlock's work, the hold and the TTI given: held = the subframes go nowhere
  void deliver(Cell& q, uint64_t upto_h, bool all);   // the measurements of segments <= upto_h (all: every one in flight) go to the loop; waits for their events
  bool inGap(int64_t lo, int64_t hi) const;
  int64_t trackedBlockInput(double max_ppm) const;   // stream_block_input with every step widened by 1 + max_ppm 1e-6: what track() and reacquire() hold the ring against
  void launchSearches();                 // the searches that are due and whose span is complete in the ring: one resampling launch into the scratches, one k_pss_acquire
  void takeSearch(Cell& q);              // the result of the cell's search goes to its TrackCell, if it was launched; waits for its event
  hipEvent_t takeEvent();
  const int device;
  const uint32_t nant, fmt;
  const LsnSampleFormat sfm;
  const size_t spb;                      // bytes of one sample of all antennas
  const uint32_t blk;
  const uint64_t ring_samples;
  int nslot = 0;
  std::vector<Cell> cells;
  std::vector<StreamCellPlan> plans;
  uint8_t* d_ring = nullptr;
  hipStream_t st_copy = nullptr, st_run = nullptr;
  hipEvent_t ev_copy = nullptr;
  std::vector<Launch> inflight;
  std::vector<hipEvent_t> ev_free;
  uint64_t pushed = 0;
  bool tracking = false, reacquiring = false, framing = false;
  std::vector<std::pair<int64_t, int64_t>> gaps;   // tracked: the gaps [lo, hi) a cell may still read
  int failed = LSN_SUCCESS;              // the first engine's failure: nothing more is submitted, every later call returns it
};

}  // namespace lsn

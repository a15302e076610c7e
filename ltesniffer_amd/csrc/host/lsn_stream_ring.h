// lsn_stream_ring.h - the object behind lsn_stream_*: the raw input of a live stream in ONE device ring, the cells' Phys fed out of it by k_resample_ring
// (DESIGN.md section 3.1g).  The counting is lsn_stream.h's; this is the part that speaks to the HIP runtime and to the engines.
#pragma once
#include "lsn_engine.h"
#include "lsn_stream.h"
#include <memory>
#include <mutex>
#include <vector>

namespace lsn {

class StreamRing {
public:
  struct CellSpec {
    Engine* e = nullptr;
    ResamplePlan plan;            // file_rate_plan's
    float offset_freq_hz = 0.0f;
    uint32_t start_tti = 0, update_meta_period = 0;
    uint64_t max_subframes = 0;
  };
  // the caller (lsn_stream_open) has checked cells, block and ring: stream_ring_check passes and blk subframes fit the Phys' block buffers
  StreamRing(int device, uint32_t nant, uint32_t fmt, float sample_scale, uint32_t blk, uint64_t ring_samples, std::vector<CellSpec> cells);
  ~StreamRing();
  int setup();                                  // ring, streams, block buffers, banks: every allocation of the stream's life
  int push(const void* iq, uint64_t n);         // iq null: a gap of n zero samples
  int flush();
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
    cf32* d_rot = nullptr;
    float* d_bank = nullptr;
    const cf32* d_nco = nullptr;
    uint64_t launches = 0;               // block buffer of launch k: slot k mod nslot ...
    uint64_t mark[NSLOT_MAX] = {};       // ... free again when the engine has consumed the chunks up to this mark (0: never used)
  };
  struct Launch { hipEvent_t ev; int64_t lo; };   // recorded behind a k_resample_ring launch that read the recording from sample lo on
  void writeRing(const uint8_t* src, uint64_t n);
  int runReady(bool flush_all);
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
  int failed = LSN_SUCCESS;              // the first engine's failure: nothing more is submitted, every later call returns it
};

}  // namespace lsn

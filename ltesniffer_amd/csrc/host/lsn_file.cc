// lsn_file.cc - replay of an IQ capture file through the engine: the file source of the reference's file mode
// (srsran_ue_sync_init_file_multi + srsran_ue_sync_zerocopy, /root/reference/src/src/LTESniffer_Core.cc:252-258,365;
// options -O / -o, ArgManager.cc:144-149).  cf32 samples (or int16 / int8 pairs: lsn_file_cfg_t.sample_format), antennas interleaved sample by sample; `offset_time` samples per
// antenna are skipped once; the stream is taken as subframe aligned (no PSS tracking in file mode), the subframe counter
// starts at start_tti; a non-zero `offset_freq` rotates every subframe by exp(-j 2 pi f n / fs), n restarting per subframe.
// A reader thread hands blocks of the file to the GPU and runs k_file_unpack on its own stream while the engine processes the
// previous blocks, so the file / PCIe leg overlaps the compute.  Default source: LSN_FILE_READERS threads pread() the block into a pinned
// buffer that lives in the engine (a 393 MB block from the page cache takes ~8 ms).  LSN_FILE_MMAP=1 selects the zero-copy variant: the
// file is mapped read-only, the pages of a block are faulted in by the same threads, the block is page-locked in place (hipHostRegister)
// and crosses PCIe straight from the page cache; on the boxes measured the lock / unlock per block costs more than the copy it saves.
// Product code: no CPU fallback, nothing from oracle/ is included or linked.
#include "lsn_engine.h"
#include "lsn_front_launch.h"
#include "lsn_cells.h"
#include <deque>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <stdexcept>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace lsn {

// block geometry of the file source: subframes per block (393 MB at 20 MHz / 2 antennas), pread threads per block, blocks in flight (one being
// read, one crossing PCIe, two in stage A; a slot is free again when stage A has consumed its block)
static void file_geometry(uint32_t& blk, uint32_t& nrd, int& nslot)
{
  blk = 800; nrd = 12; nslot = 4;
  if (const char* e = getenv("LSN_FILE_BLOCK")) blk = (uint32_t)std::max(1, atoi(e));
  if (const char* e = getenv("LSN_FILE_READERS")) nrd = (uint32_t)std::max(1, std::min(32, atoi(e)));
  if (const char* e = getenv("LSN_FILE_SLOTS")) nslot = std::max(3, std::min(8, atoi(e)));
}

void Engine::fileBlockGeometry(uint32_t& blk, int& nslot)
{
  uint32_t nrd;
  file_geometry(blk, nrd, nslot);
}

// The pinned read blocks and the device blocks of the file source (4 x 393 MB page-locked + 8 x 393 MB of HBM at 20 MHz / 2 antennas).  Page-locking
// 1.5 GB takes longer than replaying 10 000 subframes: rounds 2-4 paid it inside the first lsn_phy_process_file call (43.6 k subframes/s on the first
// pass of a 20 000-subframe capture against 96 k on the second, round-4 review).  A caller that knows it will replay a file - the reference does
// when it parses -i (LTESniffer_Core.cc:240-262) - reserves them up front with lsn_phy_prepare_file; processFile calls this as well (no-op then).
static size_t chan_buffer_bytes(uint64_t raw_samples, uint32_t nant, uint32_t L);

int Engine::reserveFileBuffers(uint32_t nof_antennas)
{
  if (!cell_set) return LSN_ERROR;
  if (nof_antennas != cd.iq_nant) return LSN_ERROR_INVALID_INPUTS;
  uint32_t blk, nrd; int nslot;
  file_geometry(blk, nrd, nslot);
  const size_t sf_bytes = (size_t)cd.sflen * nof_antennas * sizeof(cf32);
  const bool use_mmap = getenv("LSN_FILE_MMAP") && atoi(getenv("LSN_FILE_MMAP")) != 0;
  // the channel filter is set already: its intermediate for a cf32 recording and the longest filter (a replay of an integer format, whose raw block holds more
  // samples, grows it in front of its first block)
  if (chan_stopband_hz != 0.0) {
    const int r = reserveChanBuffer(chan_buffer_bytes((uint64_t)blk * cd.sflen, nof_antennas, kChanMaxL));
    if (r != LSN_SUCCESS) return r;
  }
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(cfg.device));
    for (int si = 0; si < nslot; si++) {
      FileBuf& fb = file_buf[si];
      if (fb.bytes < blk * sf_bytes) {
        if (fb.h_raw) { (void)hipHostFree(fb.h_raw); fb.h_raw = nullptr; }
        if (fb.d_raw) { (void)hipFree(fb.d_raw); fb.d_raw = nullptr; }
        if (fb.d_iq) { (void)hipFree(fb.d_iq); fb.d_iq = nullptr; }
        fb.bytes = 0;
        HIP_CHECK(hipMalloc((void**)&fb.d_raw, blk * sf_bytes));
        HIP_CHECK(hipMalloc((void**)&fb.d_iq, blk * sf_bytes));
        fb.bytes = blk * sf_bytes;
      }
      if (!use_mmap && !fb.h_raw) HIP_CHECK(hipHostMalloc((void**)&fb.h_raw, fb.bytes, hipHostMallocDefault));
    }
    return LSN_SUCCESS;
  });
}

int Engine::reserveChanBuffer(size_t bytes)
{
  if (chan_bytes >= bytes) return LSN_SUCCESS;
  if (chan_held) return LSN_ERROR_INVALID_INPUTS;   // an open stream's launches read and write d_chan
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(cfg.device));
    if (d_chan) { (void)hipFree(d_chan); d_chan = nullptr; }
    chan_bytes = 0;
    HIP_CHECK(hipMalloc((void**)&d_chan, bytes));
    chan_bytes = bytes;
    return LSN_SUCCESS;
  });
}

// the intermediate of a block whose raw buffer holds raw_samples samples per antenna: as many cf32, plus 2L
static size_t chan_buffer_bytes(uint64_t raw_samples, uint32_t nant, uint32_t L) { return (size_t)(raw_samples + 2 * (uint64_t)L) * nant * sizeof(cf32); }

int Engine::processFile(const char* path, const lsn_file_cfg_t& fc, uint32_t start_tti, uint64_t max_subframes, uint32_t update_meta_period,
                        uint64_t* subframes_done)
{
  if (antennaMap()) { if (subframes_done) *subframes_done = 0; return LSN_ERROR_INVALID_INPUTS; }   // a map is the resampler's: lsn_phy_process_file_rate
  if (chan_stopband_hz != 0.0) {   // the channel filter is set: the file is at the engine's rate and goes through both stages
    lsn_file_rate_t fr;
    fr.struct_size = sizeof(fr); fr.reserved = 0; fr.sample_rate_hz = 15000.0 * (double)cd.N; fr.offset_time_frac = 0.0; fr.center_offset_hz = 0.0;
    return processFileRate(path, fc, fr, start_tti, max_subframes, update_meta_period, subframes_done);
  }
  return processFileImpl(path, fc, nullptr, nullptr, start_tti, max_subframes, update_meta_period, subframes_done);
}

// lsn_phy_process_file_rate: a recording made at fr.sample_rate_hz.  The plan (step, start, taps, bank: lsn_resample.cc; formed by file_rate_plan, the one
// lsn_file_process_cells forms its cells' plans with) is made here, in front of everything else, so that a rate the filter does not meet is refused before a
// byte is read.
int Engine::processFileRate(const char* path, const lsn_file_cfg_t& fc, const lsn_file_rate_t& fr, uint32_t start_tti, uint64_t max_subframes,
                            uint32_t update_meta_period, uint64_t* subframes_done)
{
  if (subframes_done) *subframes_done = 0;
  if (!cell_set) return LSN_ERROR;
  // two sizes are known: the struct up to offset_time_frac (center_offset_hz reads as 0) and the whole struct
  if (fr.struct_size != offsetof(lsn_file_rate_t, center_offset_hz) && fr.struct_size != sizeof(lsn_file_rate_t)) return LSN_ERROR_INVALID_INPUTS;
  const double center = fr.struct_size == sizeof(lsn_file_rate_t) ? fr.center_offset_hz : 0.0;
  if (fc.offset_time_samples < 0 || !(fr.offset_time_frac >= 0.0 && fr.offset_time_frac < 4.0e18)) return LSN_ERROR_INVALID_INPUTS;
  if (const lsn_antenna_map_t* m = antennaMap()) {   // always through the resampler, equal rates too; fc.nof_antennas is the recording's
    if (chan_stopband_hz != 0.0) return LSN_ERROR_INVALID_INPUTS;   // (limit: no channel filter with a map)
    ResamplePlan plan;
    const int r = file_rate_plan_map(fr.sample_rate_hz, cd.N, cd.nof_prb, fc.offset_time_samples, fr.offset_time_frac, center, fc.nof_antennas, m->nof_out, m->src_antenna,
                                     m->offset_hz, plan);
    if (r != LSN_SUCCESS) return r;
    return processFileImpl(path, fc, &plan, nullptr, start_tti, max_subframes, update_meta_period, subframes_done);
  }
  if (fr.sample_rate_hz == 15000.0 * (double)cd.N && fr.offset_time_frac == 0.0 && center == 0.0 && chan_stopband_hz == 0.0)
    return processFileImpl(path, fc, nullptr, nullptr, start_tti, max_subframes, update_meta_period, subframes_done);
  // with the channel filter set the mixer runs in stage 1 and the resampler, stage 2, is the plan of the same pair and start with no offset
  ChanFilter filt;
  const bool filtered = chan_stopband_hz != 0.0;
  if (filtered) {
    const int rf = filt.init(fr.sample_rate_hz, 15000.0 * (6.0 * (double)cd.nof_prb + 1.0), chan_stopband_hz, center);
    if (rf != LSN_SUCCESS) return rf;
  }
  ResamplePlan plan;
  const int r = file_rate_plan(fr.sample_rate_hz, cd.N, cd.nof_prb, fc.offset_time_samples, fr.offset_time_frac, filtered ? 0.0 : center, plan);
  if (r != LSN_SUCCESS) return r;
  return processFileImpl(path, fc, &plan, filtered ? &filt : nullptr, start_tti, max_subframes, update_meta_period, subframes_done);
}

// One replay of one file into the engines of `cells`: one cell (lsn_phy_process_file[_rate]) or several (lsn_file_process_cells).  A cell's rs is
// the resampler's plan, or null (single-cell call only): the file is at the engine's rate and k_file_unpack converts it.  With plans, block k of OUTPUT
// subframes of every cell is fed from the union of the input samples the cells read (lsn_cells.h - neighbouring blocks overlap by the filter length), read once and
// copied once, and k_resample (one cell) or k_resample_cells (several: one launch, each cell into its own engine's block buffer) takes the place of k_file_unpack.
// The struct owns what the replay opens (file, mapping, stream, rotation tables, resampler banks, page-locked ranges, reader thread) and its destructor gives it
// back, whichever way the replay ends.
struct Engine::FileReplay {
  static constexpr int NSLOT_MAX = 8;
  struct Cell {
    Engine* e = nullptr;
    const ResamplePlan* rs = nullptr;
    uint32_t sflen = 0;
    float offset_freq_hz = 0.0f;
    uint32_t start_tti = 0, update_meta_period = 0;
    uint64_t max_subframes = 0;
    uint64_t sf_in_file = 0, first_sf = 0, done = 0;   // complete subframes in the file / in front of the replay (DECODE_MIB state of the reference) / submitted
    // the -o rotation and, with rs, the resampler's bank and NCO tables (a few hundred kB, as short-lived as the replay); front.cf: stage 1 in front of rs, raw block
    // -> the engine's intermediate (y1 over the span rs reads) -> rs, or null: rs reads the raw block.  The tables go with the cell: ~FileReplay clears the cells, whose
    // engines it has waited for, before it destroys the stream
    FrontCell front;
    int rc = LSN_SUCCESS;         // what this cell's engine answered (submit, then wait)
  };
  struct Slot { cf32* h_raw = nullptr; cf32* d_raw = nullptr; cf32* d_iq[kFileMaxCells] = {}; uint32_t nsf[kFileMaxCells] = {}; uint64_t mark[kFileMaxCells] = {};
                int state = 0; /* 0 free, 1 ready, 2 eof */ void* reg = nullptr; /* page-locked range of the file mapping this block is copied from */ };
  std::vector<Cell> cells;
  Engine& e;                   // the first cell's: device, reader-thread pinning
  Engine* big = nullptr;       // the engine whose block buffers are largest: the raw block (pinned and device) of a slot is its
  const uint32_t nant, fmt;    // nant: the RECORDING's antennas - what is read and what the raw block holds; a cell's block buffers have its Phy's
  const LsnSampleFormat sfm;   // bytes of one complex sample in the file (the block buffers are sized for cf32, the widest) and the conversion's scale
  const size_t spb;            // bytes of one sample of all antennas
  size_t sf_bytes = 0;         // single cell at the engine's rate: bytes of one subframe ...
  const uint64_t file_off0;    // ... and where subframe 0 starts
  uint32_t blk, nrd;           // subframes per block, page-touch / pread threads per block
  uint32_t blk_geom = 0;       // blk as file_geometry gave it: what the block buffers are sized for
  size_t raw_bytes = 0;        // bytes a raw block buffer holds: blk_geom subframes of cf32 of the cell whose Phy has the largest blocks (subframe length x ITS antennas)
  int NSLOT;                   // blocks in flight (round 2 held eight until their chunks were written - and paid 8 x 393 MB of pinned allocation on the first call)
  int fd = -1; size_t file_size = 0;
  bool use_mmap = false;  // measured on MI355X boxes (page-cache file): pread into pinned blocks 60 k subframes/s, in-place locking 26 k (lock / unlock per block)
  uint8_t* map = nullptr; const long page = sysconf(_SC_PAGESIZE);
  hipStream_t st = nullptr;
  Slot slot[NSLOT_MAX];
  std::vector<FileCellPlan> plans;              // what the reader cuts blocks from (plan(), behind scanMib)
  std::mutex fm; std::condition_variable fcv;   // slot states, reader <-> submit loop
  std::string rerr; bool abort_reader = false; std::thread reader;
  const bool fdebug = getenv("LSN_FILE_DEBUG") != nullptr;
  const double t_begin = now_ms();

  FileReplay(const lsn_file_cfg_t& fc, const FileCellJob* jobs, uint32_t n)
      : e(*jobs[0].e), nant(fc.nof_antennas), fmt(fc.sample_format), sfm(lsn_sample_format(fc.sample_format, fc.sample_scale)), spb((size_t)nant * sfm.bytes),
        file_off0((uint64_t)fc.offset_time_samples * nant * sfm.bytes)
  {
    file_geometry(blk, nrd, NSLOT);
    blk_geom = blk;
    size_t widest = 0;   // samples of all antennas of one subframe of a Phy
    for (uint32_t c = 0; c < n; c++) {
      Cell k;
      k.e = jobs[c].e; k.rs = jobs[c].rs; k.front.cf = jobs[c].cf; k.sflen = k.e->cd.sflen; k.offset_freq_hz = jobs[c].offset_freq_hz; k.start_tti = jobs[c].start_tti;
      k.update_meta_period = jobs[c].update_meta_period; k.max_subframes = jobs[c].max_subframes;
      if ((size_t)k.sflen * k.e->cd.iq_nant > widest) { widest = (size_t)k.sflen * k.e->cd.iq_nant; big = k.e; }
      cells.push_back(std::move(k));
    }
    sf_bytes = (size_t)cells[0].sflen * nant * sfm.bytes;
    raw_bytes = (size_t)blk_geom * widest * sizeof(cf32);
  }

  ~FileReplay()
  {
    { std::unique_lock<std::mutex> lk(fm); abort_reader = true; }
    fcv.notify_all();
    if (reader.joinable()) reader.join();
    for (auto& s : slot) if (s.reg) (void)hipHostUnregister(s.reg);
    cells.clear();   // the cells' tables go before the stream does
    if (st) (void)hipStreamDestroy(st);
    if (map) munmap(map, file_size);
    if (fd >= 0) close(fd);
  }

  bool resampled() const { return cells[0].rs != nullptr; }   // (several cells: every one has a plan)
  bool filtered() const { return cells[0].front.cf != nullptr; }    // (several cells: all or none, lsn_file_process_cells)

  // the cells as lsn_cells.h wants them, from where each one starts
  void plan()
  {
    plans.clear();
    for (auto& c : cells) {
      FileCellPlan p;
      p.rs = c.rs; p.pre = c.front.cf ? c.front.cf->L : 0; p.sflen = c.sflen; p.first_sf = c.first_sf; p.total = file_cell_total(c.sf_in_file, c.first_sf, c.max_subframes);
      plans.push_back(p);
    }
  }

  // the block buffers are sized for blk_geom subframes of cf32 at the OUTPUT rate of the widest cell: a block carries as many subframes as have the union of their
  // input fit.  false: not one subframe of every cell - the starts lie too far apart (or LSN_FILE_BLOCK is too small for one subframe's input)
  bool fitBlock()
  {
    plan();
    const uint32_t fit = file_cells_fit(plans.data(), (uint32_t)plans.size(), blk_geom, raw_bytes / spb);
    if (!fit) {
      if (cells.size() > 1) fprintf(stderr, "ltesniffer_amd: the cells' start positions lie too far apart for one block of %u subframes: pass start positions closer together, or replay the cells separately\n", blk_geom);
      return false;
    }
    blk = fit;
    return true;
  }

  // the file, how many subframes of every cell it holds, the block size that fits, the mapping (LSN_FILE_MMAP)
  int open(const char* path)
  {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) return LSN_ERROR_INVALID_INPUTS;
    struct stat sb;
    if (fstat(fd, &sb)) return LSN_ERROR_INVALID_INPUTS;
    file_size = (size_t)sb.st_size;
    for (auto& c : cells) {
      const uint64_t in_end = (uint64_t)file_size / spb;
      if (c.rs) c.sf_in_file = c.rs->outputsInside(c.front.cf ? c.front.cf->insideEnd(in_end) : in_end) / c.sflen;  // output subframes whose whole input span lies inside the file
      else c.sf_in_file = (uint64_t)file_size > file_off0 ? ((uint64_t)file_size - file_off0) / sf_bytes : 0;  // complete subframes only
    }
    if (resampled() && !fitBlock()) return LSN_ERROR_INVALID_INPUTS;
    if (const char* v = getenv("LSN_FILE_MMAP")) use_mmap = atoi(v) != 0;
    if (use_mmap && file_size > 0) {
      void* m = mmap(nullptr, file_size, PROT_READ, MAP_SHARED, fd, 0);
      if (m == MAP_FAILED) use_mmap = false; else map = (uint8_t*)m;
    } else {
      use_mmap = false;
    }
    return LSN_SUCCESS;
  }

  // the cells [c0, c1) through the chain (lsn_front_launch.h): nsf[c] subframes from output subframe sf0[c], out of the raw samples [lo, lo + len) of the recording
  // into out[c], queued on st
  void queueFront(size_t c0, size_t c1, const void* raw, int64_t lo, uint64_t len, const uint64_t* sf0, const uint32_t* nsf, cf32* const* out)
  {
    const FrontCell* fc[kFileMaxCells];
    LsnResampleCell k[kFileMaxCells];
    int64_t in_lo[kFileMaxCells] = {}, in_hi[kFileMaxCells] = {};
    for (size_t c = c0; c < c1; c++) {
      const Cell& q = cells[c];
      fc[c - c0] = &q.front;
      k[c - c0] = q.rs->cell(sf0[c] * q.sflen, q.sflen, q.front.tb, out[c], (uint64_t)nsf[c] * q.sflen);
      if (nsf[c]) q.rs->inputSpan(sf0[c] * q.sflen, (uint64_t)nsf[c] * q.sflen, in_lo[c - c0], in_hi[c - c0]);
    }
    lsn_launch_front({raw, fmt, sfm.scale, lo, len, nant, 0}, fc, k, in_lo, in_hi, (uint32_t)(c1 - c0), st, "file source: a block");
  }

  // the conversion of a block, raw block -> [subframe][antenna][sample] cf32 of every cell that takes part, queued on st
  void queueConvert(Slot& s, const FileCellsBlock& b)
  {
    if (!resampled()) { lsn_launch_file_unpack(s.d_raw, fmt, sfm.scale, cells[0].front.tb.d_rot, cells[0].sflen, nant, s.d_iq[0], b.nsf[0], st); return; }
    queueFront(0, cells.size(), s.d_raw, b.in_lo, (uint64_t)(b.in_hi - b.in_lo), b.sf0, b.nsf, s.d_iq);
  }

  // stream, block buffers (kept by the engines: no-op when lsn_phy_prepare_file or an earlier call made them), rotation tables, resampler banks and NCO tables -
  // of all cells, once, in front of the first block
  void setup()
  {
    HIP_CHECK(hipSetDevice(e.cfg.device));
    HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto& c : cells)
      if (c.e->reserveFileBuffers(c.e->cd.iq_nant) != LSN_SUCCESS) throw std::runtime_error("file source: block buffers");
    for (int si = 0; si < NSLOT; si++) {
      Slot& s = slot[si];
      FileBuf& fb = big->file_buf[si];
      if (fb.bytes < raw_bytes) throw std::runtime_error("file source: raw block buffer");
      s.h_raw = fb.h_raw; s.d_raw = fb.d_raw;
      for (size_t c = 0; c < cells.size(); c++) s.d_iq[c] = cells[c].e->file_buf[si].d_iq;
    }
    for (auto& c : cells) {
      FrontCell& f = c.front;
      f.tb.rotation(c.offset_freq_hz, c.sflen, 15000.0 * (double)c.e->cd.N);
      if (c.rs) f.tb.upload(*c.rs, st);
      if (f.cf) {   // the intermediate: reserved by lsn_phy_prepare_file when the filter was set by then, otherwise here - in front of the first block, never inside the loop
        f.ft.upload(*f.cf, st);
        if (c.e->reserveChanBuffer(chan_buffer_bytes(raw_bytes / spb, nant, f.cf->L)) != LSN_SUCCESS) throw std::runtime_error("file source: channel filter buffer");
        f.mid = c.e->chanBuffer(); f.mid_cap = c.e->chanBufferSamples(nant);
      }
    }
    if (resampled()) HIP_CHECK(hipStreamSynchronize(st));
  }

  // LSN_TTI_FROM_MIB of cell ci: the first subframe 0 within 64 radio frames whose MIB decodes -> its first_sf and the TTI its replay starts with; false: none
  bool scanMib(size_t ci)
  {
    Cell& c = cells[ci];
    for (uint64_t i = 0; i < c.sf_in_file && i < 10 * 64; i += 10) {  // the file starts at subframe 0 of a radio frame (file mode has no sync)
      int64_t lo = 0, hi = 0;
      if (c.rs) { c.rs->inputSpan(i * c.sflen, c.sflen, lo, hi); if (c.front.cf) c.front.cf->widen(lo, hi); lo = std::max<int64_t>(lo, 0); }
      const uint64_t len = c.rs ? (uint64_t)(hi - lo) : c.sflen;
      const size_t bytes = c.rs ? (size_t)len * spb : sf_bytes;
      if (bytes > raw_bytes) throw std::runtime_error("file source: one subframe's input does not fit the block buffer");
      std::vector<uint8_t> one(bytes);
      if (pread(fd, one.data(), bytes, (off_t)(c.rs ? (uint64_t)lo * spb : file_off0 + i * sf_bytes)) != (ssize_t)bytes) break;
      HIP_CHECK(hipMemcpyAsync(slot[0].d_raw, one.data(), bytes, hipMemcpyHostToDevice, st));
      HIP_CHECK(hipStreamSynchronize(st));
      if (c.rs) { uint64_t sf0[kFileMaxCells] = {}; uint32_t one_sf[kFileMaxCells] = {}; sf0[ci] = i; one_sf[ci] = 1; queueFront(ci, ci + 1, slot[0].d_raw, lo, len, sf0, one_sf, slot[0].d_iq); }   // one cell of several: a one-cell launch
      else lsn_launch_file_unpack(slot[0].d_raw, fmt, sfm.scale, c.front.tb.d_rot, c.sflen, nant, slot[0].d_iq[ci], 1, st);
      HIP_CHECK(hipStreamSynchronize(st));
      lsn_mib_t mib;
      const int r = c.e->mibDecode(slot[0].d_iq[ci], true, &mib, nullptr);
      if (r < 0) throw std::runtime_error("MIB decode failed");
      if (r == 1) { c.first_sf = i; c.start_tti = mib.sfn * 10u; return true; }
    }
    return false;
  }

  // the bytes [0, total) in nrd pieces of `part`, each by a thread of its own: body(piece, first byte, end)
  template <class F>
  void splitOver(size_t total, size_t part, F&& body)
  {
    std::vector<std::thread> rd;
    for (uint32_t r = 0; r < nrd; r++) {
      const size_t b0 = std::min(total, (size_t)r * part), b1 = std::min(total, b0 + part);
      if (b0 == b1) continue;
      rd.emplace_back([&body, r, b0, b1] { body(r, b0, b1); });
    }
    for (auto& t : rd) t.join();
  }

  // the `total` bytes of a block that start at byte boff of the file -> where the H2D copy reads them: the page-locked mapping, else the slot's pinned buffer
  const uint8_t* readBlock(Slot& s, uint64_t boff, size_t total)
  {
    const size_t part = (total / nrd + 4095) & ~(size_t)4095;
    const double tb0 = now_ms();
    if (use_mmap) {
      // fault the pages of the block in (page-cache hits: a page-table walk per page; otherwise this is the read-ahead), then lock them
      const uint8_t* b = map + boff;
      uint8_t* lo = (uint8_t*)((uintptr_t)b & ~(uintptr_t)(page - 1));
      const size_t len = (size_t)(b + total - lo);
      (void)madvise(lo, len, MADV_WILLNEED);
      std::vector<unsigned> sink(nrd, 0);
      splitOver(len, part, [&](uint32_t r, size_t b0, size_t b1) { unsigned a = 0; for (size_t o = b0; o < b1; o += (size_t)page) a += lo[o]; sink[r] = a; });
      const double tr0 = now_ms();
      const bool ok = hipHostRegister(lo, len, hipHostRegisterDefault) == hipSuccess;
      if (fdebug) fprintf(stderr, "lsn_file: block at %.1f ms: touch %.1f ms, register %.1f ms (%s)\n", tb0 - t_begin, tr0 - tb0, now_ms() - tr0, ok ? "ok" : "failed");
      if (ok) { s.reg = lo; return b; }
      (void)hipGetLastError();  // this mapping cannot be page-locked: copy through pinned buffers from here on
      use_mmap = false;
    }
    if (!s.h_raw) { FileBuf& fb = big->file_buf[&s - slot]; HIP_CHECK(hipHostMalloc((void**)&fb.h_raw, fb.bytes, hipHostMallocDefault)); s.h_raw = fb.h_raw; }
    // the page-cache copy of one thread tops out near 9 GB/s: split the block over a few pread()ers
    std::vector<int> bad(nrd, 0);
    splitOver(total, part, [&](uint32_t r, size_t b0, size_t b1) {
      size_t o = b0;
      while (o < b1) {
        const ssize_t k = pread(fd, (char*)s.h_raw + o, b1 - o, (off_t)(boff + o));
        if (k <= 0) { bad[r] = 1; return; }
        o += (size_t)k;
      }
    });
    for (int b : bad) if (b) throw std::runtime_error("read failed");
    if (fdebug) fprintf(stderr, "lsn_file: block at %.1f ms: pread %.1f ms\n", tb0 - t_begin, now_ms() - tb0);
    return (const uint8_t*)s.h_raw;
  }

  // block b into slot s: ONE read, then ONE copy and the conversion QUEUED on st - the submits are ordered behind them on the device, so the reader goes
  // straight on to the next block while this one crosses PCIe
  void queueBlock(Slot& s, const FileCellsBlock& b)
  {
    const bool rs = resampled();   // the block's input samples are [in_lo, in_hi) of the recording, else whole subframes from file_off0
    const size_t total = rs ? (size_t)(b.in_hi - b.in_lo) * spb : b.nsf[0] * sf_bytes;
    if (total > raw_bytes) throw std::runtime_error("file source: a block's input does not fit the block buffer");
    const uint8_t* src = readBlock(s, rs ? (uint64_t)b.in_lo * spb : file_off0 + b.sf0[0] * sf_bytes, total);
    HIP_CHECK(hipMemcpyAsync(s.d_raw, src, total, hipMemcpyHostToDevice, st));
    queueConvert(s, b);
  }

  // reader thread: fills the free slots in turn until every cell is through the file (or its max_subframes); an empty block marks the end
  void readerLoop()
  {
    try {
      (void)hipSetDevice(e.cfg.device);
      e.pinThisThread(nullptr);
      uint64_t k = 0;
      for (int i = 0;; i = (i + 1) % NSLOT, k++) {
        Slot& s = slot[i];
        {
          std::unique_lock<std::mutex> lk(fm);
          fcv.wait(lk, [&] { return s.state == 0 || abort_reader; });
          if (abort_reader) return;
        }
        FileCellsBlock b;
        const bool got = file_cells_block(plans.data(), (uint32_t)plans.size(), blk, k, b);
        if (s.reg) { (void)hipHostUnregister(s.reg); s.reg = nullptr; }  // the block this slot carried last has been committed
        if (got) queueBlock(s, b);
        {
          std::unique_lock<std::mutex> lk(fm);
          for (size_t c = 0; c < cells.size(); c++) s.nsf[c] = b.nsf[c];
          s.state = got ? 1 : 2;
        }
        fcv.notify_all();
        if (!got) return;
      }
    } catch (const std::exception& ex) {
      std::unique_lock<std::mutex> lk(fm);
      rerr = ex.what();
      for (auto& s : slot) if (s.state == 0) s.state = 2;
      fcv.notify_all();
    }
  }

  // block i is submitted (searched, queued for decoding) to every engine that takes part in it, in cell order, while block i-1 drains; its slot goes back to the
  // reader once every chunk of it has been through stage A of every one of them.  An engine that fails ends the submitting for all; all are waited for.
  int submitLoop()
  {
    int rc = LSN_SUCCESS;
    std::deque<int> inflight;  // submitted blocks whose slot the reader may not touch yet (pinned source + device buffers still in use)
    for (int i = 0;; i = (i + 1) % NSLOT) {
      Slot& s = slot[i];
      {
        std::unique_lock<std::mutex> lk(fm);
        fcv.wait(lk, [&] { return s.state != 0; });
        if (s.state == 2) break;
      }
      for (size_t ci = 0; ci < cells.size(); ci++) {
        Cell& c = cells[ci];
        // behind a failure: not submitted, nothing to wait for.  The slot of the failing block goes into `inflight` like any other and the loop ends: it is never
        // handed back to the reader - its copy and kernel may still be on the stream - and is given up with the replay (the destructor joins the reader first)
        if (rc != LSN_SUCCESS) s.nsf[ci] = 0;
        if (!s.nsf[ci]) continue;
        c.rc = c.e->submit(s.d_iq[ci], s.nsf[ci], (uint32_t)((c.start_tti + c.done) % 10240u), c.update_meta_period, st);
        s.mark[ci] = c.e->submitMark();
        c.done += s.nsf[ci];
        if (c.rc != LSN_SUCCESS) rc = c.rc;
      }
      inflight.push_back(i);
      while ((int)inflight.size() > NSLOT - 2) {  // keep two slots for the reader, hand the oldest one back once its chunks are written
        const int o = inflight.front();
        inflight.pop_front();
        for (size_t ci = 0; ci < cells.size(); ci++)   // stage A has read the block (UL_MODE: its chunks are written): pinned source and device buffers are free
          if (slot[o].nsf[ci]) cells[ci].e->waitIqConsumed(slot[o].mark[ci]);
        { std::unique_lock<std::mutex> lk(fm); slot[o].state = 0; }
        fcv.notify_all();
      }
      if (rc != LSN_SUCCESS) break;
    }
    for (auto& c : cells) {
      const int w = c.e->wait();
      if (c.rc == LSN_SUCCESS) c.rc = w;
      if (rc == LSN_SUCCESS) rc = c.rc;
    }
    return rc;
  }
};

// the replay of `n` cells (FileCellJob: engine, plan, start) of one file; the single-cell entry points are its n = 1 case
int Engine::replayFile(const char* path, const lsn_file_cfg_t& fc, FileCellJob* jobs, uint32_t n)
{
  FileReplay f(fc, jobs, n);
  int rc = f.open(path);
  if (rc != LSN_SUCCESS) return rc;
  try {
    f.setup();
    bool moved = false;
    for (size_t c = 0; c < f.cells.size(); c++) {
      if (f.cells[c].start_tti != LSN_TTI_FROM_MIB) continue;
      if (!f.scanMib(c)) throw std::runtime_error("no MIB found in the first 64 radio frames of the file");
      moved = true;
    }
    if (moved && f.resampled() && !f.fitBlock()) return LSN_ERROR_INVALID_INPUTS;   // the MIBs put the cells' starts too far apart
    f.plan();
    if (f.fdebug) fprintf(stderr, "lsn_file: setup %.1f ms, mmap %d, %zu cell(s), block %u subframes, %d slots, %u readers\n", now_ms() - f.t_begin, (int)f.use_mmap, f.cells.size(), f.blk, f.NSLOT, f.nrd);
    f.reader = std::thread([&] { f.readerLoop(); });
    rc = f.submitLoop();
    if (f.fdebug) fprintf(stderr, "lsn_file: %llu subframes (first cell) done at %.1f ms\n", (unsigned long long)f.cells[0].done, now_ms() - f.t_begin);
    if (!f.rerr.empty()) throw std::runtime_error(f.rerr);
  } catch (const std::exception& ex) {
    fprintf(stderr, "ltesniffer_amd: %s\n", ex.what());
    rc = LSN_ERROR;
  }
  for (uint32_t c = 0; c < n; c++) { jobs[c].done = f.cells[c].done; jobs[c].status = f.cells[c].rc; }
  return rc;
}

int Engine::processFileImpl(const char* path, const lsn_file_cfg_t& fc, const ResamplePlan* rs, const ChanFilter* cf, uint32_t start_tti, uint64_t max_subframes, uint32_t update_meta_period,
                            uint64_t* subframes_done)
{
  if (subframes_done) *subframes_done = 0;
  if (!cell_set) return LSN_ERROR;
  // a mapped plan reads a recording of any 1 .. 8 antennas (its sources were checked against fc.nof_antennas when it was formed); every other replay the Phy's own
  const bool mapped = rs && rs->map_nout;
  if (mapped ? (fc.nof_antennas < 1 || fc.nof_antennas > 8 || rs->map_nout != cd.iq_nant) : fc.nof_antennas != cd.iq_nant) return LSN_ERROR_INVALID_INPUTS;
  if (!path || fc.offset_time_samples < 0 || !lsn_sample_format(fc.sample_format, fc.sample_scale).valid) return LSN_ERROR_INVALID_INPUTS;
  FileCellJob job;
  job.e = this; job.rs = rs; job.cf = cf; job.offset_freq_hz = fc.offset_freq_hz; job.start_tti = start_tti; job.update_meta_period = update_meta_period; job.max_subframes = max_subframes;
  const int rc = replayFile(path, fc, &job, 1);
  if (subframes_done) *subframes_done = job.done;
  return rc;
}

}  // namespace lsn

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
#include "lsn_resample.h"
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

// The pinned read blocks and the device blocks of the file source (4 x 393 MB page-locked + 8 x 393 MB of HBM at 20 MHz / 2 antennas).  Page-locking
// 1.5 GB takes longer than replaying 10 000 subframes: rounds 2-4 paid it inside the first lsn_phy_process_file call (43.6 k subframes/s on the first
// pass of a 20 000-subframe capture against 96 k on the second, round-4 review).  A caller that knows it will replay a file - the reference does
// when it parses -i (LTESniffer_Core.cc:240-262) - reserves them up front with lsn_phy_prepare_file; processFile calls this as well (no-op then).
int Engine::reserveFileBuffers(uint32_t nof_antennas)
{
  if (!cell_set) return LSN_ERROR;
  if (nof_antennas != cd.iq_nant) return LSN_ERROR_INVALID_INPUTS;
  uint32_t blk, nrd; int nslot;
  file_geometry(blk, nrd, nslot);
  const size_t sf_bytes = (size_t)cd.sflen * nof_antennas * sizeof(cf32);
  const bool use_mmap = getenv("LSN_FILE_MMAP") && atoi(getenv("LSN_FILE_MMAP")) != 0;
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

int Engine::processFile(const char* path, const lsn_file_cfg_t& fc, uint32_t start_tti, uint64_t max_subframes, uint32_t update_meta_period,
                        uint64_t* subframes_done)
{
  return processFileImpl(path, fc, nullptr, start_tti, max_subframes, update_meta_period, subframes_done);
}

// lsn_phy_process_file_rate: a recording made at fr.sample_rate_hz.  The plan (step, start, taps, bank: lsn_resample.cc) is made here, in front of
// everything else, so that a rate the filter does not meet is refused before a byte is read.
int Engine::processFileRate(const char* path, const lsn_file_cfg_t& fc, const lsn_file_rate_t& fr, uint32_t start_tti, uint64_t max_subframes,
                            uint32_t update_meta_period, uint64_t* subframes_done)
{
  if (subframes_done) *subframes_done = 0;
  if (!cell_set) return LSN_ERROR;
  // two sizes are known: the struct up to offset_time_frac (center_offset_hz reads as 0) and the whole struct
  if (fr.struct_size != offsetof(lsn_file_rate_t, center_offset_hz) && fr.struct_size != sizeof(lsn_file_rate_t)) return LSN_ERROR_INVALID_INPUTS;
  const double center = fr.struct_size == sizeof(lsn_file_rate_t) ? fr.center_offset_hz : 0.0;
  if (fc.offset_time_samples < 0 || !(fr.offset_time_frac >= 0.0 && fr.offset_time_frac < 4.0e18)) return LSN_ERROR_INVALID_INPUTS;
  const double rate_out = 15000.0 * (double)cd.N, whole = std::floor(fr.offset_time_frac);
  if (fr.sample_rate_hz == rate_out && fr.offset_time_frac == 0.0 && center == 0.0) return processFileImpl(path, fc, nullptr, start_tti, max_subframes, update_meta_period, subframes_done);
  const uint64_t first = (uint64_t)fc.offset_time_samples + (uint64_t)whole;
  ResamplePlan plan;
  const int r = plan.init(fr.sample_rate_hz, rate_out, 15000.0 * (6.0 * (double)cd.nof_prb + 1.0), first, fr.offset_time_frac - whole, center);
  if (r != LSN_SUCCESS) return r;
  return processFileImpl(path, fc, &plan, start_tti, max_subframes, update_meta_period, subframes_done);
}

// One replay: rs is the resampler's plan (processFileRate), or null: the file is at the engine's rate.  With a plan, block k of OUTPUT subframes is fed
// from the input samples it reads (ResamplePlan::inputSpan - neighbouring blocks overlap by the filter length), and k_resample takes the place of
// k_file_unpack.  The struct owns what the replay opens (file, mapping, stream, rotation table, resampler bank, page-locked ranges, reader thread) and its
// destructor gives it back, whichever way the replay ends.
struct Engine::FileReplay {
  static constexpr int NSLOT_MAX = 8;
  struct Slot { cf32* h_raw = nullptr; cf32* d_raw = nullptr; cf32* d_iq = nullptr; uint32_t nsf = 0; int state = 0; /* 0 free, 1 ready, 2 eof */ uint64_t mark = 0;
                void* reg = nullptr; /* page-locked range of the file mapping this block is copied from */ };
  Engine& e;
  const ResamplePlan* const rs;
  const uint32_t nant, sflen, fmt;
  const LsnSampleFormat sfm;   // bytes of one complex sample in the file (the block buffers are sized for cf32, the widest) and the conversion's scale
  const size_t sf_bytes, spb;  // bytes of one subframe / of one sample of all antennas
  const uint64_t file_off0;
  const float offset_freq_hz;
  uint32_t blk, nrd;           // subframes per block, page-touch / pread threads per block
  int NSLOT;                   // blocks in flight (round 2 held eight until their chunks were written - and paid 8 x 393 MB of pinned allocation on the first call)
  int fd = -1; size_t file_size = 0;
  uint64_t sf_in_file = 0, first_sf = 0, done = 0;   // complete subframes in the file / in front of the replay (DECODE_MIB state of the reference) / submitted
  bool use_mmap = false;  // measured on MI355X boxes (page-cache file): pread into pinned blocks 60 k subframes/s, in-place locking 26 k (lock / unlock per block)
  uint8_t* map = nullptr; const long page = sysconf(_SC_PAGESIZE);
  cf32* d_rot = nullptr;
  float* d_bank = nullptr;      // the resampler's bank (a few hundred kB, as short-lived as d_rot) ...
  const cf32* d_nco = nullptr;  // ... and, behind it in the same allocation, the mixer's tables when the plan has a tuning word
  hipStream_t st = nullptr;
  Slot slot[NSLOT_MAX];
  std::mutex fm; std::condition_variable fcv;   // slot states, reader <-> submit loop
  std::string rerr; bool abort_reader = false; std::thread reader;
  const bool fdebug = getenv("LSN_FILE_DEBUG") != nullptr;
  const double t_begin = now_ms();

  FileReplay(Engine& eng, const lsn_file_cfg_t& fc, const ResamplePlan* plan)
      : e(eng), rs(plan), nant(fc.nof_antennas), sflen(eng.cd.sflen), fmt(fc.sample_format), sfm(lsn_sample_format(fc.sample_format, fc.sample_scale)),
        sf_bytes((size_t)sflen * nant * sfm.bytes), spb((size_t)nant * sfm.bytes), file_off0((uint64_t)fc.offset_time_samples * nant * sfm.bytes),
        offset_freq_hz(fc.offset_freq_hz) { file_geometry(blk, nrd, NSLOT); }

  ~FileReplay()
  {
    { std::unique_lock<std::mutex> lk(fm); abort_reader = true; }
    fcv.notify_all();
    if (reader.joinable()) reader.join();
    for (auto& s : slot) if (s.reg) (void)hipHostUnregister(s.reg);
    if (d_rot) (void)hipFree(d_rot);
    if (d_bank) (void)hipFree(d_bank);
    if (st) (void)hipStreamDestroy(st);
    if (map) munmap(map, file_size);
    if (fd >= 0) close(fd);
  }

  // the file, how many subframes it holds, the block size that fits, the mapping (LSN_FILE_MMAP)
  int open(const char* path)
  {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) return LSN_ERROR_INVALID_INPUTS;
    struct stat sb;
    if (fstat(fd, &sb)) return LSN_ERROR_INVALID_INPUTS;
    file_size = (size_t)sb.st_size;
    sf_in_file = (uint64_t)file_size > file_off0 ? ((uint64_t)file_size - file_off0) / sf_bytes : 0;  // complete subframes only
    if (rs) {
      sf_in_file = rs->outputsInside((uint64_t)file_size / spb) / sflen;  // output subframes whose whole input span lies inside the file
      // the block buffers are sized for blk subframes of cf32 at the OUTPUT rate: a block carries as many subframes as have their input fit
      const u128 cap = (u128)blk * sflen * sizeof(cf32) / sfm.bytes;
      const u128 fit = cap > rs->taps + 2 ? ((cap - rs->taps - 2) << 64) / ((u128)sflen * rs->step) : 0;
      if (fit == 0) return LSN_ERROR_INVALID_INPUTS;
      if (fit < blk) blk = (uint32_t)fit;
    }
    if (const char* v = getenv("LSN_FILE_MMAP")) use_mmap = atoi(v) != 0;
    if (use_mmap && file_size > 0) {
      void* m = mmap(nullptr, file_size, PROT_READ, MAP_SHARED, fd, 0);
      if (m == MAP_FAILED) use_mmap = false; else map = (uint8_t*)m;
    } else {
      use_mmap = false;
    }
    return LSN_SUCCESS;
  }

  // input of the output subframes [pos, pos + n): first sample (zeros in front of the file are the kernel's), number of samples
  void rsSpan(uint64_t pos, uint64_t n, int64_t& lo, uint64_t& len) const
  {
    int64_t hi;
    rs->inputSpan(pos * sflen, n * sflen, lo, hi);
    lo = std::max<int64_t>(lo, 0);
    len = hi > lo ? (uint64_t)(hi - lo) : 0;
  }

  // the conversion of n subframes from position pos, raw block -> [subframe][antenna][sample] cf32, queued on st
  void queueConvert(const void* raw, int64_t lo, uint64_t len, uint64_t pos, uint32_t n, cf32* out)
  {
    if (!rs) { lsn_launch_file_unpack(raw, fmt, sfm.scale, d_rot, sflen, nant, out, n, st); return; }
    const u128 base = rs->position(pos * sflen);
    lsn_launch_resample(raw, fmt, sfm.scale, lo, len, (uint64_t)(base >> 64), (uint64_t)base, (uint32_t)(rs->step >> 64), (uint64_t)rs->step, rs->taps, rs->span, d_bank, rs->tune,
                        d_nco, d_rot, sflen, 0, nant, out, (uint64_t)n * sflen, st);
  }

  // stream, block buffers (kept by the engine: no-op when lsn_phy_prepare_file or an earlier call made them), rotation table, resampler bank
  void setup()
  {
    HIP_CHECK(hipSetDevice(e.cfg.device));
    HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (e.reserveFileBuffers(nant) != LSN_SUCCESS) throw std::runtime_error("file source: block buffers");
    for (int si = 0; si < NSLOT; si++) {
      Slot& s = slot[si];
      FileBuf& fb = e.file_buf[si];
      s.h_raw = fb.h_raw; s.d_raw = fb.d_raw; s.d_iq = fb.d_iq;
    }
    if (offset_freq_hz != 0.0f) {
      std::vector<cf32> rot(sflen);
      const double fs = 15000.0 * (double)e.cd.N;
      for (uint32_t n = 0; n < sflen; n++) {
        const double a = -2.0 * M_PI * (double)offset_freq_hz * (double)n / fs;
        rot[n] = {(float)std::cos(a), (float)std::sin(a)};
      }
      HIP_CHECK(hipMalloc((void**)&d_rot, sflen * sizeof(cf32)));
      HIP_CHECK(hipMemcpy(d_rot, rot.data(), sflen * sizeof(cf32), hipMemcpyHostToDevice));
    }
    if (rs) {
      rs->upload(d_bank, d_nco, st);
      HIP_CHECK(hipStreamSynchronize(st));
    }
  }

  // LSN_TTI_FROM_MIB: the first subframe 0 within 64 radio frames whose MIB decodes -> first_sf and the TTI the replay starts with; false: none
  bool scanMib(uint32_t& start_tti)
  {
    for (uint64_t i = 0; i < sf_in_file && i < 10 * 64; i += 10) {  // the file starts at subframe 0 of a radio frame (file mode has no sync)
      int64_t lo = 0; uint64_t len = sflen;
      if (rs) rsSpan(i, 1, lo, len);
      const size_t bytes = rs ? (size_t)len * spb : sf_bytes;
      std::vector<uint8_t> one(bytes);
      if (pread(fd, one.data(), bytes, (off_t)(rs ? (uint64_t)lo * spb : file_off0 + i * sf_bytes)) != (ssize_t)bytes) break;
      HIP_CHECK(hipMemcpyAsync(slot[0].d_raw, one.data(), bytes, hipMemcpyHostToDevice, st));
      HIP_CHECK(hipStreamSynchronize(st));
      queueConvert(slot[0].d_raw, lo, len, i, 1, slot[0].d_iq);
      HIP_CHECK(hipStreamSynchronize(st));
      lsn_mib_t mib;
      const int r = e.mibDecode(slot[0].d_iq, true, &mib, nullptr);
      if (r < 0) throw std::runtime_error("MIB decode failed");
      if (r == 1) { first_sf = i; start_tti = mib.sfn * 10u; return true; }
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
    if (!s.h_raw) { FileBuf& fb = e.file_buf[&s - slot]; HIP_CHECK(hipHostMalloc((void**)&fb.h_raw, fb.bytes, hipHostMallocDefault)); s.h_raw = fb.h_raw; }
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

  // `got` subframes from position pos into slot s: read, then copy and conversion QUEUED on st - the submit is ordered behind them on the device, so the
  // reader goes straight on to the next block while this one crosses PCIe
  void queueBlock(Slot& s, uint64_t pos, uint32_t got)
  {
    int64_t in_lo = 0; uint64_t in_len = 0;   // resampler: the block's input samples [in_lo, in_lo + in_len)
    if (rs) rsSpan(pos, got, in_lo, in_len);
    const size_t total = rs ? (size_t)in_len * spb : got * sf_bytes;
    const uint8_t* src = readBlock(s, rs ? (uint64_t)in_lo * spb : file_off0 + pos * sf_bytes, total);
    HIP_CHECK(hipMemcpyAsync(s.d_raw, src, total, hipMemcpyHostToDevice, st));
    queueConvert(s.d_raw, in_lo, in_len, pos, got, s.d_iq);
  }

  // reader thread: fills the free slots in turn until the file (or max_subframes) is through; an empty block marks the end
  void readerLoop(uint64_t max_subframes)
  {
    try {
      (void)hipSetDevice(e.cfg.device);
      e.pinThisThread(nullptr);
      uint64_t avail = sf_in_file - first_sf, left = max_subframes ? std::min<uint64_t>(max_subframes, avail) : avail, pos = first_sf;
      for (int i = 0;; i = (i + 1) % NSLOT) {
        Slot& s = slot[i];
        {
          std::unique_lock<std::mutex> lk(fm);
          fcv.wait(lk, [&] { return s.state == 0 || abort_reader; });
          if (abort_reader) return;
        }
        const uint32_t got = (uint32_t)std::min<uint64_t>(blk, left);
        if (s.reg) { (void)hipHostUnregister(s.reg); s.reg = nullptr; }  // the block this slot carried last has been committed
        if (got) queueBlock(s, pos, got);
        pos += got;
        left -= got;
        { std::unique_lock<std::mutex> lk(fm); s.nsf = got; s.state = got ? 1 : 2; }
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

  // block i is submitted (searched, queued for decoding) while block i-1 drains; its slot goes back to the reader once every chunk
  // of it has been through stage A
  int submitLoop(uint32_t start_tti, uint32_t update_meta_period)
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
      rc = e.submit(s.d_iq, s.nsf, (uint32_t)((start_tti + done) % 10240u), update_meta_period, st);
      s.mark = e.submitMark();
      done += s.nsf;
      inflight.push_back(i);
      while ((int)inflight.size() > NSLOT - 2) {  // keep two slots for the reader, hand the oldest one back once its chunks are written
        const int o = inflight.front();
        inflight.pop_front();
        e.waitIqConsumed(slot[o].mark);  // stage A has read the block (UL_MODE: its chunks are written): pinned source and device buffers are free
        { std::unique_lock<std::mutex> lk(fm); slot[o].state = 0; }
        fcv.notify_all();
      }
      if (rc != LSN_SUCCESS) break;
    }
    const int w = e.wait();
    return rc == LSN_SUCCESS ? w : rc;
  }
};

int Engine::processFileImpl(const char* path, const lsn_file_cfg_t& fc, const ResamplePlan* rs, uint32_t start_tti, uint64_t max_subframes, uint32_t update_meta_period,
                            uint64_t* subframes_done)
{
  if (subframes_done) *subframes_done = 0;
  if (!cell_set) return LSN_ERROR;
  if (!path || fc.nof_antennas != cd.iq_nant || fc.offset_time_samples < 0 || !lsn_sample_format(fc.sample_format, fc.sample_scale).valid) return LSN_ERROR_INVALID_INPUTS;
  FileReplay f(*this, fc, rs);
  int rc = f.open(path);
  if (rc != LSN_SUCCESS) return rc;
  try {
    f.setup();
    if (start_tti == LSN_TTI_FROM_MIB && !f.scanMib(start_tti)) throw std::runtime_error("no MIB found in the first 64 radio frames of the file");
    if (f.fdebug) fprintf(stderr, "lsn_file: setup %.1f ms, mmap %d, block %u subframes, %d slots, %u readers\n", now_ms() - f.t_begin, (int)f.use_mmap, f.blk, f.NSLOT, f.nrd);
    f.reader = std::thread([&] { f.readerLoop(max_subframes); });
    rc = f.submitLoop(start_tti, update_meta_period);
    if (f.fdebug) fprintf(stderr, "lsn_file: %llu subframes done at %.1f ms\n", (unsigned long long)f.done, now_ms() - f.t_begin);
    if (!f.rerr.empty()) throw std::runtime_error(f.rerr);
  } catch (const std::exception& ex) {
    fprintf(stderr, "ltesniffer_amd: %s\n", ex.what());
    rc = LSN_ERROR;
  }
  if (subframes_done) *subframes_done = f.done;
  return rc;
}

}  // namespace lsn

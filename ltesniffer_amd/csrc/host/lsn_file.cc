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
#include <chrono>
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

#define HIP_CHECK(x)                                                                                       \
  do {                                                                                                     \
    hipError_t _e = (x);                                                                                   \
    if (_e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #x); \
  } while (0)

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
  try {
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
  } catch (const std::exception& ex) {
    fprintf(stderr, "ltesniffer_amd: %s\n", ex.what());
    return LSN_ERROR;
  }
  return LSN_SUCCESS;
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

// rs: the resampler's plan (processFileRate), or null: the file is at the engine's rate.  With a plan, block k of OUTPUT subframes is fed from the input
// samples it reads (ResamplePlan::inputSpan - neighbouring blocks overlap by the filter length), and k_resample takes the place of k_file_unpack.
int Engine::processFileImpl(const char* path, const lsn_file_cfg_t& fc, const ResamplePlan* rs, uint32_t start_tti, uint64_t max_subframes, uint32_t update_meta_period,
                            uint64_t* subframes_done)
{
  if (subframes_done) *subframes_done = 0;
  if (!cell_set) return LSN_ERROR;
  if (!path || fc.nof_antennas != cd.iq_nant || fc.offset_time_samples < 0 || fc.sample_format > LSN_FILE_SC8) return LSN_ERROR_INVALID_INPUTS;
  if (fc.sample_format != LSN_FILE_CF32 && !(fc.sample_scale >= 0.0f && fc.sample_scale < INFINITY)) return LSN_ERROR_INVALID_INPUTS;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return LSN_ERROR_INVALID_INPUTS;
  struct stat sb;
  if (fstat(fd, &sb)) { close(fd); return LSN_ERROR_INVALID_INPUTS; }
  const uint32_t nant = fc.nof_antennas, sflen = cd.sflen, fmt = fc.sample_format;
  // bytes of one complex sample in the file; the block buffers are sized for cf32, the widest
  const size_t smp_bytes = fmt == LSN_FILE_SC16 ? 4 : fmt == LSN_FILE_SC8 ? 2 : sizeof(cf32);
  const float smp_scale = fmt == LSN_FILE_CF32 ? 1.0f : fc.sample_scale != 0.0f ? fc.sample_scale : fmt == LSN_FILE_SC16 ? 1.0f / 32768.0f : 1.0f / 128.0f;
  const size_t sf_bytes = (size_t)sflen * nant * smp_bytes;
  uint32_t blk, nrd;  // subframes per block, page-touch / pread threads per block
  int NSLOT;          // blocks in flight (round 2 held eight until their chunks were written - and paid 8 x 393 MB of pinned allocation on the first call)
  file_geometry(blk, nrd, NSLOT);
  const uint64_t file_off0 = (uint64_t)fc.offset_time_samples * nant * smp_bytes;
  uint64_t sf_in_file = (uint64_t)sb.st_size > file_off0 ? ((uint64_t)sb.st_size - file_off0) / sf_bytes : 0;  // complete subframes only
  const size_t spb = (size_t)nant * smp_bytes;  // bytes of one sample of all antennas
  if (rs) {
    sf_in_file = rs->outputsInside((uint64_t)sb.st_size / spb) / sflen;  // output subframes whose whole input span lies inside the file
    // the block buffers are sized for blk subframes of cf32 at the OUTPUT rate: a block carries as many subframes as have their input fit
    const u128 cap = (u128)blk * sflen * sizeof(cf32) / smp_bytes;
    const u128 fit = cap > rs->taps + 2 ? ((cap - rs->taps - 2) << 64) / ((u128)sflen * rs->step) : 0;
    if (fit == 0) { close(fd); return LSN_ERROR_INVALID_INPUTS; }
    if (fit < blk) blk = (uint32_t)fit;
  }
  // input of the output subframes [pos, pos + n): first sample (zeros in front of the file are the kernel's), number of samples
  auto rs_span = [&](uint64_t pos, uint64_t n, int64_t& lo, uint64_t& len) {
    int64_t hi;
    rs->inputSpan(pos * sflen, n * sflen, lo, hi);
    lo = std::max<int64_t>(lo, 0);
    len = hi > lo ? (uint64_t)(hi - lo) : 0;
  };
  auto rs_launch = [&](const void* raw, int64_t lo, uint64_t len, uint64_t pos, uint32_t n, const float* bank, const cf32* nco, const cf32* rot, cf32* out, hipStream_t s) {
    const u128 base = rs->position(pos * sflen);
    lsn_launch_resample(raw, fmt, smp_scale, lo, len, (uint64_t)(base >> 64), (uint64_t)base, (uint32_t)(rs->step >> 64), (uint64_t)rs->step, rs->taps, rs->span, bank, rs->tune, nco, rot,
                        sflen, 0, nant, out, (uint64_t)n * sflen, s);
  };
  constexpr int NSLOT_MAX = 8;
  const bool fdebug = getenv("LSN_FILE_DEBUG") != nullptr;
  auto tnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_begin = tnow();
  struct Slot { cf32* h_raw = nullptr; cf32* d_raw = nullptr; cf32* d_iq = nullptr; uint32_t nsf = 0; int state = 0; /* 0 free, 1 ready, 2 eof */ uint64_t mark = 0;
                void* reg = nullptr; /* page-locked range of the file mapping this block is copied from */ } slot[NSLOT_MAX];
  bool use_mmap = false;  // measured on MI355X boxes (page-cache file): pread into pinned blocks 60 k subframes/s, in-place locking 26 k (lock / unlock per block)
  if (const char* e = getenv("LSN_FILE_MMAP")) use_mmap = atoi(e) != 0;
  uint8_t* map = nullptr;
  const long page = sysconf(_SC_PAGESIZE);
  if (use_mmap && sb.st_size > 0) {
    void* m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_SHARED, fd, 0);
    if (m == MAP_FAILED) use_mmap = false; else map = (uint8_t*)m;
  } else {
    use_mmap = false;
  }
  cf32* d_rot = nullptr;
  float* d_bank = nullptr;  // the resampler's bank (a few hundred kB, as short-lived as d_rot) ...
  const cf32* d_nco = nullptr;  // ... and, behind it in the same allocation, the mixer's tables when the plan has a tuning word
  hipStream_t st = nullptr;
  std::mutex fm;
  std::condition_variable fcv;
  std::string rerr;
  bool abort_reader = false;
  int rc = LSN_SUCCESS;
  uint64_t done = 0;
  std::thread reader;
  try {
    HIP_CHECK(hipSetDevice(cfg.device));
    HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (reserveFileBuffers(nant) != LSN_SUCCESS) throw std::runtime_error("file source: block buffers");  // (kept by the engine: no-op when lsn_phy_prepare_file or an earlier call made them)
    for (int si = 0; si < NSLOT; si++) {
      Slot& s = slot[si];
      FileBuf& fb = file_buf[si];
      s.h_raw = fb.h_raw; s.d_raw = fb.d_raw; s.d_iq = fb.d_iq;
    }
    if (fc.offset_freq_hz != 0.0f) {
      std::vector<cf32> rot(sflen);
      const double fs = 15000.0 * (double)cd.N;
      for (uint32_t n = 0; n < sflen; n++) {
        const double a = -2.0 * M_PI * (double)fc.offset_freq_hz * (double)n / fs;
        rot[n] = {(float)std::cos(a), (float)std::sin(a)};
      }
      HIP_CHECK(hipMalloc((void**)&d_rot, sflen * sizeof(cf32)));
      HIP_CHECK(hipMemcpy(d_rot, rot.data(), sflen * sizeof(cf32), hipMemcpyHostToDevice));
    }
    if (rs) {
      rs->upload(d_bank, d_nco, st);
      HIP_CHECK(hipStreamSynchronize(st));
    }
    uint64_t first_sf = 0;  // subframes of the file in front of the replay (DECODE_MIB state of the reference)
    if (start_tti == LSN_TTI_FROM_MIB) {
      bool found = false;
      for (uint64_t i = 0; i < sf_in_file && i < 10 * 64; i += 10) {  // the file starts at subframe 0 of a radio frame (file mode has no sync)
        int64_t lo = 0;
        uint64_t len = sflen;
        if (rs) rs_span(i, 1, lo, len);
        const size_t bytes = rs ? (size_t)len * spb : sf_bytes;
        std::vector<uint8_t> one(bytes);
        if (pread(fd, one.data(), bytes, (off_t)(rs ? (uint64_t)lo * spb : file_off0 + i * sf_bytes)) != (ssize_t)bytes) break;
        HIP_CHECK(hipMemcpyAsync(slot[0].d_raw, one.data(), bytes, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (rs) rs_launch(slot[0].d_raw, lo, len, i, 1, d_bank, d_nco, d_rot, slot[0].d_iq, st);
        else lsn_launch_file_unpack(slot[0].d_raw, fmt, smp_scale, d_rot, sflen, nant, slot[0].d_iq, 1, st);
        HIP_CHECK(hipStreamSynchronize(st));
        lsn_mib_t mib;
        const int r = mibDecode(slot[0].d_iq, true, &mib, nullptr);
        if (r < 0) throw std::runtime_error("MIB decode failed");
        if (r == 1) { found = true; first_sf = i; start_tti = mib.sfn * 10u; break; }
      }
      if (!found) { rc = LSN_ERROR; throw std::runtime_error("no MIB found in the first 64 radio frames of the file"); }
    }
    if (fdebug) fprintf(stderr, "lsn_file: setup %.1f ms, mmap %d, block %u subframes, %d slots, %u readers\n", tnow() - t_begin, (int)use_mmap, blk, NSLOT, nrd);
    reader = std::thread([&] {
      try {
        (void)hipSetDevice(cfg.device);
        pinThisThread(nullptr);
        uint64_t avail = sf_in_file - first_sf, left = max_subframes ? std::min<uint64_t>(max_subframes, avail) : avail, pos = first_sf;
        for (int i = 0;; i = (i + 1) % NSLOT) {
          Slot& s = slot[i];
          {
            std::unique_lock<std::mutex> lk(fm);
            fcv.wait(lk, [&] { return s.state == 0 || abort_reader; });
            if (abort_reader) return;
          }
          const size_t got = (size_t)std::min<uint64_t>(blk, left);
          const double tb0 = tnow();
          if (s.reg) { (void)hipHostUnregister(s.reg); s.reg = nullptr; }  // the block this slot carried last has been committed
          if (got) {
            int64_t in_lo = 0;   // resampler: the block's input samples [in_lo, in_lo + in_len)
            uint64_t in_len = 0;
            if (rs) rs_span(pos, got, in_lo, in_len);
            const size_t total = rs ? (size_t)in_len * spb : got * sf_bytes, part = (total / nrd + 4095) & ~(size_t)4095;
            const uint64_t boff = rs ? (uint64_t)in_lo * spb : file_off0 + pos * sf_bytes;  // first byte of the block in the file
            const uint8_t* src = nullptr;
            if (use_mmap) {
              // fault the pages of the block in (page-cache hits: a page-table walk per page; otherwise this is the read-ahead), then lock them
              const uint8_t* b = map + boff;
              uint8_t* lo = (uint8_t*)((uintptr_t)b & ~(uintptr_t)(page - 1));
              const size_t len = (size_t)(b + total - lo);
              (void)madvise(lo, len, MADV_WILLNEED);
              std::vector<std::thread> rd;
              std::vector<unsigned> sink(nrd, 0);
              for (uint32_t r = 0; r < nrd; r++) {
                const size_t b0 = std::min(len, (size_t)r * part), b1 = std::min(len, b0 + part);
                if (b0 == b1) continue;
                rd.emplace_back([&, r, b0, b1] { unsigned a = 0; for (size_t o = b0; o < b1; o += (size_t)page) a += lo[o]; sink[r] = a; });
              }
              for (auto& t : rd) t.join();
              const double tr0 = tnow();
              if (hipHostRegister(lo, len, hipHostRegisterDefault) == hipSuccess) { s.reg = lo; src = b; }
              if (fdebug) fprintf(stderr, "lsn_file: block at %.1f ms: touch %.1f ms, register %.1f ms (%s)\n", tb0 - t_begin, tr0 - tb0, tnow() - tr0, src ? "ok" : "failed");
              if (!src) {  // this mapping cannot be page-locked: copy through pinned buffers from here on
                (void)hipGetLastError();
                use_mmap = false;
              }
            }
            if (!src) {
              if (!s.h_raw) { FileBuf& fb = file_buf[&s - slot]; HIP_CHECK(hipHostMalloc((void**)&fb.h_raw, fb.bytes, hipHostMallocDefault)); s.h_raw = fb.h_raw; }
              // the page-cache copy of one thread tops out near 9 GB/s: split the block over a few pread()ers
              std::vector<std::thread> rd;
              std::vector<int> bad(nrd, 0);
              for (uint32_t r = 0; r < nrd; r++) {
                const size_t b0 = std::min(total, (size_t)r * part), b1 = std::min(total, b0 + part);
                if (b0 == b1) continue;
                rd.emplace_back([&, r, b0, b1] {
                  size_t o = b0;
                  while (o < b1) {
                    const ssize_t k = pread(fd, (char*)s.h_raw + o, b1 - o, (off_t)(boff + o));
                    if (k <= 0) { bad[r] = 1; return; }
                    o += (size_t)k;
                  }
                });
              }
              for (auto& t : rd) t.join();
              for (int b : bad) if (b) throw std::runtime_error("read failed");
              src = (const uint8_t*)s.h_raw;
              if (fdebug) fprintf(stderr, "lsn_file: block at %.1f ms: pread %.1f ms\n", tb0 - t_begin, tnow() - tb0);
            }
            // the copy and the de-interleave are only QUEUED here (stream st); the submit below is ordered behind them on the device, so
            // the reader goes straight on to the next block while this one crosses PCIe
            HIP_CHECK(hipMemcpyAsync(s.d_raw, src, total, hipMemcpyHostToDevice, st));
            if (rs) rs_launch(s.d_raw, in_lo, in_len, pos, (uint32_t)got, d_bank, d_nco, d_rot, s.d_iq, st);
            else lsn_launch_file_unpack(s.d_raw, fmt, smp_scale, d_rot, sflen, nant, s.d_iq, (uint32_t)got, st);
            pos += got;
          }
          left -= got;
          {
            std::unique_lock<std::mutex> lk(fm);
            s.nsf = (uint32_t)got;
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
    });
    // block i is submitted (searched, queued for decoding) while block i-1 drains; its slot goes back to the reader once every chunk
    // of it has been through stage A
    std::deque<int> inflight;  // submitted blocks whose slot the reader may not touch yet (pinned source + device buffers still in use)
    for (int i = 0;; i = (i + 1) % NSLOT) {
      Slot& s = slot[i];
      {
        std::unique_lock<std::mutex> lk(fm);
        fcv.wait(lk, [&] { return s.state != 0; });
        if (s.state == 2) break;
      }
      rc = submit(s.d_iq, s.nsf, (uint32_t)((start_tti + done) % 10240u), update_meta_period, st);
      s.mark = submitMark();
      done += s.nsf;
      inflight.push_back(i);
      while ((int)inflight.size() > NSLOT - 2) {  // keep two slots for the reader, hand the oldest one back once its chunks are written
        const int o = inflight.front();
        inflight.pop_front();
        waitIqConsumed(slot[o].mark);  // stage A has read the block (UL_MODE: its chunks are written): pinned source and device buffers are free
        { std::unique_lock<std::mutex> lk(fm); slot[o].state = 0; }
        fcv.notify_all();
      }
      if (rc != LSN_SUCCESS) break;
    }
    {
      const int w = wait();
      if (rc == LSN_SUCCESS) rc = w;
    }
    if (fdebug) fprintf(stderr, "lsn_file: %llu subframes done at %.1f ms\n", (unsigned long long)done, tnow() - t_begin);
    if (!rerr.empty()) throw std::runtime_error(rerr);
  } catch (const std::exception& ex) {
    fprintf(stderr, "ltesniffer_amd: %s\n", ex.what());
    rc = LSN_ERROR;
  }
  {
    std::unique_lock<std::mutex> lk(fm);
    abort_reader = true;
  }
  fcv.notify_all();
  if (reader.joinable()) reader.join();
  for (auto& s : slot) {
    if (s.reg) (void)hipHostUnregister(s.reg);
  }
  if (d_rot) (void)hipFree(d_rot);
  if (d_bank) (void)hipFree(d_bank);
  if (st) (void)hipStreamDestroy(st);
  if (map) munmap(map, (size_t)sb.st_size);
  close(fd);
  if (subframes_done) *subframes_done = done;
  return rc;
}

}  // namespace lsn

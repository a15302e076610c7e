// lsn_stream_ring.cc - a live wideband stream pushed in host buffers (lsn_stream_*).  The raw input lives in one device ring of
// ring_samples samples per antenna, recording sample n at slot n & (ring_samples - 1); a push copies its samples host-to-device straight to their slots (no host
// staging buffer, no memcpy on the caller's thread), a gap is a hipMemsetAsync of the same slots.  Whenever a cell has a block of complete subframes
// (lsn_stream.h: the file replay's counting), ONE k_resample_ring launch resamples every such cell out of the ring into a block buffer of its Phy - the ones the
// file source uses, recycled with submitMark / waitIqConsumed as FileReplay does - and the block is submitted.  An output sample is a function of (input,
// configuration, m) only (section 3.1b), so the Phys get the samples of the file replay of the same bytes however the stream was cut.
// Two HIP streams: copies and memsets on one, launches on the other.  A launch waits for the copies queued so far; a piece that is written over slots an
// unfinished launch may still read waits on the event recorded behind that launch, and on nothing else.  Product code: no CPU fallback.
#include "lsn_stream_ring.h"
#include "lsn_resample_launch.h"
#include <algorithm>
#include <cmath>

namespace lsn {

StreamRing::StreamRing(int device_, uint32_t nant_, uint32_t fmt_, float sample_scale, uint32_t blk_, uint64_t ring_samples_, std::vector<CellSpec> specs)
    : device(device_), nant(nant_), fmt(fmt_), sfm(lsn_sample_format(fmt_, sample_scale)), spb((size_t)nant_ * sfm.bytes), blk(blk_), ring_samples(ring_samples_)
{
  for (auto& s : specs) {
    Cell c;
    c.s = std::move(s);
    c.sflen = c.s.e->sfLen();
    cells.push_back(std::move(c));
  }
  // (the plans point into cells, which does not grow any more)
  for (auto& c : cells) {
    StreamCellPlan p;
    p.rs = &c.s.plan; p.sflen = c.sflen; p.max_subframes = c.s.max_subframes;
    plans.push_back(p);
  }
}

StreamRing::~StreamRing()
{
  (void)hipSetDevice(device);
  for (auto& c : cells) (void)c.s.e->wait();   // nothing of this stream's is in an engine any more ...
  if (st_copy) (void)hipStreamSynchronize(st_copy);
  if (st_run) (void)hipStreamSynchronize(st_run);   // ... or on the device
  for (auto& l : inflight) (void)hipEventDestroy(l.ev);
  for (auto& e : ev_free) (void)hipEventDestroy(e);
  if (ev_copy) (void)hipEventDestroy(ev_copy);
  for (auto& c : cells) {
    if (c.d_rot) (void)hipFree(c.d_rot);
    if (c.d_bank) (void)hipFree(c.d_bank);
  }
  if (d_ring) (void)hipFree(d_ring);
  if (st_copy) (void)hipStreamDestroy(st_copy);
  if (st_run) (void)hipStreamDestroy(st_run);
}

int StreamRing::setup()
{
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    uint32_t blk_geom;
    Engine::fileBlockGeometry(blk_geom, nslot);
    nslot = std::min(nslot, NSLOT_MAX);
    if (blk > blk_geom) return LSN_ERROR_INVALID_INPUTS;
    HIP_CHECK(hipStreamCreateWithFlags(&st_copy, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&st_run, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&ev_copy, hipEventDisableTiming));
    HIP_CHECK(hipMalloc((void**)&d_ring, (size_t)ring_samples * spb));
    for (auto& c : cells) {
      const int r = c.s.e->reserveFileBuffers(nant);
      if (r != LSN_SUCCESS) return r;
      for (int si = 0; si < nslot; si++)
        if (c.s.e->fileIqBlockBytes(si) < (size_t)blk * c.sflen * nant * sizeof(cf32)) throw std::runtime_error("stream: block buffer");
      if (c.s.offset_freq_hz != 0.0f) {   // the -o rotation of the cell's output samples, as the file source forms it
        std::vector<cf32> rot(c.sflen);
        const double fs = 15000.0 * (double)c.s.e->symbolSz();
        for (uint32_t n = 0; n < c.sflen; n++) {
          const double a = -2.0 * M_PI * (double)c.s.offset_freq_hz * (double)n / fs;
          rot[n] = {(float)std::cos(a), (float)std::sin(a)};
        }
        HIP_CHECK(hipMalloc((void**)&c.d_rot, c.sflen * sizeof(cf32)));
        HIP_CHECK(hipMemcpy(c.d_rot, rot.data(), c.sflen * sizeof(cf32), hipMemcpyHostToDevice));
      }
      c.s.plan.upload(c.d_bank, c.d_nco, st_run);
    }
    HIP_CHECK(hipStreamSynchronize(st_run));
    return LSN_SUCCESS;
  });
}

int64_t StreamRing::oldestNeeded() const
{
  uint64_t done[kFileMaxCells];
  for (size_t c = 0; c < cells.size(); c++) done[c] = cells[c].done;
  return stream_oldest_needed(plans.data(), (uint32_t)plans.size(), done, pushed);
}

hipEvent_t StreamRing::takeEvent()
{
  hipEvent_t ev = nullptr;
  if (!ev_free.empty()) { ev = ev_free.back(); ev_free.pop_back(); }
  else HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  return ev;
}

// n samples (src null: zeros) to the slots of recording samples [pushed, pushed + n): the caller has cut the piece so that it neither crosses the end of the ring
// nor reaches a sample a cell still needs
void StreamRing::writeRing(const uint8_t* src, uint64_t n)
{
  const int64_t over_end = (int64_t)(pushed + n) - (int64_t)ring_samples;   // the recording samples in front of it lose their slots
  for (size_t i = 0; i < inflight.size();) {
    Launch& l = inflight[i];
    const hipError_t q = hipEventQuery(l.ev);
    if (q == hipSuccess) {   // finished: its event goes back
      ev_free.push_back(l.ev);
      inflight[i] = inflight.back();
      inflight.pop_back();
      continue;
    }
    if (q != hipErrorNotReady) HIP_CHECK(q);
    (void)hipGetLastError();
    if (l.lo < over_end) HIP_CHECK(hipStreamWaitEvent(st_copy, l.ev, 0));
    i++;
  }
  uint8_t* dst = d_ring + (size_t)(pushed & (ring_samples - 1)) * spb;
  if (src) HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)n * spb, hipMemcpyHostToDevice, st_copy));
  else HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)n * spb, st_copy));
}

// every launch that is due: one k_resample_ring for the cells that have a block, then one submit per such cell in the order of the list
int StreamRing::runReady(bool flush_all)
{
  for (;;) {
    if (failed != LSN_SUCCESS) return failed;
    uint32_t nsf[kFileMaxCells] = {};
    int64_t in_lo = 0, in_hi = 0;
    bool any = false;
    for (size_t c = 0; c < cells.size(); c++) {
      nsf[c] = stream_cell_ready(plans[c], pushed, cells[c].done, blk, flush_all);
      if (!nsf[c]) continue;
      int64_t lo, hi;
      cells[c].s.plan.inputSpan(cells[c].done * cells[c].sflen, (uint64_t)nsf[c] * cells[c].sflen, lo, hi);
      in_lo = any ? std::min(in_lo, lo) : lo;
      in_hi = any ? std::max(in_hi, hi) : hi;
      any = true;
    }
    if (!any) return LSN_SUCCESS;
    in_lo = std::max<int64_t>(in_lo, 0);   // zeros in front of the stream are the kernel's
    if (in_hi > (int64_t)pushed || (uint64_t)(in_hi - in_lo) > ring_samples || (int64_t)pushed - in_lo > (int64_t)ring_samples)
      throw std::runtime_error("stream: a block's input is not in the ring");
    LsnResampleCell k[kFileMaxCells];
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      k[c] = LsnResampleCell();
      if (!nsf[c]) continue;
      const int si = (int)(q.launches % (uint64_t)nslot);
      if (q.mark[si]) q.s.e->waitIqConsumed(q.mark[si]);   // the block this buffer carried last has been through stage A
      const u128 base = q.s.plan.position(q.done * q.sflen);
      k[c].base_hi = (uint64_t)(base >> 64); k[c].base_lo = (uint64_t)base; k[c].d_lo = (uint64_t)q.s.plan.step; k[c].d_hi = (uint32_t)(q.s.plan.step >> 64);
      k[c].taps = q.s.plan.taps; k[c].span = q.s.plan.span; k[c].sflen = q.sflen; k[c].sf_off = 0; k[c].bank = q.d_bank; k[c].w = q.s.plan.tune; k[c].nco = q.d_nco; k[c].rot = q.d_rot;
      k[c].out = q.s.e->fileIqBlock(si); k[c].n_out = (uint64_t)nsf[c] * q.sflen;
    }
    HIP_CHECK(hipEventRecord(ev_copy, st_copy));
    HIP_CHECK(hipStreamWaitEvent(st_run, ev_copy, 0));   // the samples pushed so far are in their slots
    lsn_launch_resample_ring(d_ring, ring_samples, fmt, sfm.scale, in_lo, (uint64_t)(in_hi - in_lo), nant, k, (uint32_t)cells.size(), st_run);
    Launch l;
    l.ev = takeEvent(); l.lo = in_lo;
    HIP_CHECK(hipEventRecord(l.ev, st_run));
    inflight.push_back(l);
    for (size_t c = 0; c < cells.size() && failed == LSN_SUCCESS; c++) {
      Cell& q = cells[c];
      if (!nsf[c]) continue;
      const int si = (int)(q.launches % (uint64_t)nslot);
      q.rc = q.s.e->submit(k[c].out, nsf[c], (uint32_t)((q.s.start_tti + q.done) % 10240u), q.s.update_meta_period, st_run);
      q.mark[si] = q.s.e->submitMark();
      q.launches++;
      q.done += nsf[c];
      if (q.rc != LSN_SUCCESS) failed = q.rc;   // nothing more is submitted to any Phy
    }
  }
}

int StreamRing::push(const void* iq, uint64_t n)
{
  if (failed != LSN_SUCCESS) return failed;
  if (n >= (1ull << 62) || pushed + n >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  const int r = guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    const uint8_t* src = (const uint8_t*)iq;
    while (n && failed == LSN_SUCCESS) {
      // a piece ends at the end of the ring, and in front of the slot of the oldest sample a cell still needs.  No cell has a block left to submit here, so the
      // cell that holds that sample waits for data inside its own block's span, which the ring holds (stream_ring_check): there is room
      const uint64_t held = pushed - (uint64_t)oldestNeeded();
      if (held >= ring_samples) throw std::runtime_error("stream: the ring is full of samples no cell can use yet");
      const uint64_t take = std::min(n, std::min(ring_samples - held, ring_samples - (pushed & (ring_samples - 1))));
      writeRing(src, take);
      pushed += take;
      if (src) src += (size_t)take * spb;
      n -= take;
      (void)runReady(false);
    }
    HIP_CHECK(hipStreamSynchronize(st_copy));   // the samples are in the ring: the caller's buffer is free
    return failed;
  });
  if (r != LSN_SUCCESS && failed == LSN_SUCCESS) failed = r;
  return r;
}

int StreamRing::flush()
{
  if (failed != LSN_SUCCESS) return failed;
  const int r = guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    (void)runReady(true);
    for (auto& c : cells) {   // all are waited for, whatever one of them answered
      const int w = c.s.e->wait();
      if (c.rc == LSN_SUCCESS) c.rc = w;
      if (failed == LSN_SUCCESS) failed = c.rc;
    }
    return failed;
  });
  if (r != LSN_SUCCESS && failed == LSN_SUCCESS) failed = r;
  return r;
}

}  // namespace lsn

// lsn_stream_ring.cc - a live wideband stream pushed in host buffers (lsn_stream_*).  The raw input lives in one device ring of
// ring_samples samples per antenna, recording sample n at slot n & (ring_samples - 1); a push copies its samples host-to-device straight to their slots (no host
// staging buffer, no memcpy on the caller's thread), a gap is a hipMemsetAsync of the same slots.  Whenever a cell has a block of complete subframes
// (lsn_stream.h: the file replay's counting), ONE k_resample_ring launch resamples every such cell out of the ring into a block buffer of its Phy - the ones the
// file source uses, recycled with submitMark / waitIqConsumed as FileReplay does - and the block is submitted.  An output sample is a function of (input,
// configuration, m) only (section 3.1b), so the Phys get the samples of the file replay of the same bytes however the stream was cut.
// Two HIP streams: copies and memsets on one, launches on the other.  A launch waits for the copies queued so far; a piece that is written over slots an
// unfinished launch may still read waits on the event recorded behind that launch, and on nothing else.  Product code: no CPU fallback.
// A stream that asked for it (track()) follows the sample clock: runReadyTracked resamples segment by segment at the steps its timing loop
// decides (lsn_track.h) and measures every segment's PSS with k_pss_timing; a stream that did not runs runReady exactly as before.  The two loops differ in how a
// block buffer fills; what they do alike - bufferFor, launchRing, submitBlock - exists once.
// A tracked stream that asked for it too (reacquire()) searches a cell whose loop has lost the PSS over a whole half frame: launchSearches
// resamples the span into a scratch of the cell's and runs k_pss_acquire on it - launches of their own, which a stream that loses nothing never issues -, and the
// enter() of three segments later moves the position once.
// With frameSync() on top the first subframe of every segment of a running check goes through the PBCH decode of its Phy's side scratch,
// queued on st_run directly behind the segment's k_pss_timing window; the result rides with the measurement (Cell::Pending) and the rule in lsn_track.cc decides the
// TTI from it.  Where the counting or the hold changes, the block buffer is closed first: no block spans two countings.
// Cells with a channel filter: the chain launchRing queues (lsn_launch_front, the one the file source queues: section 3.1l) runs both stages -
// one k_chan_fir_ring launch out of the ring into the cells' intermediates, one k_resample per cell out of those - and every span that guards the ring is L samples
// wider on both sides.  Without one, nothing differs.
#include "lsn_stream_ring.h"
#include "lsn_track_launch.h"
#include "lsn_clock.h"
#include <algorithm>
#include <cmath>
#include <cstring>

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
    p.rs = &c.s.plan; p.sflen = c.sflen; p.max_subframes = c.s.max_subframes; p.pre = c.s.filt.L;
    plans.push_back(p);
    c.front.cf = &c.s.filt;
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
    if (c.d_rep) (void)hipFree(c.d_rep);
    if (c.front.mid) c.s.e->holdChanBuffer(false);   // (mid is the Phy's: given back, not freed)
    if (c.h_C) (void)hipHostFree(c.h_C);
    if (c.acq_x) (void)hipFree(c.acq_x);
    if (c.acq_C) (void)hipHostFree(c.acq_C);
    if (c.acq_ev) (void)hipEventDestroy(c.acq_ev);
    if (c.h_cand) (void)hipHostFree(c.h_cand);
    for (auto& p : c.pending) if (p.ev) (void)hipEventDestroy(p.ev);
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
      // the ring holds the STREAM's antennas (nant); a cell's block buffers hold its Phy's - the same number unless the cell has an antenna map
      const uint32_t rows = c.s.e->iqAntennas();
      const int r = c.s.e->reserveFileBuffers(rows);
      if (r != LSN_SUCCESS) return r;
      for (int si = 0; si < nslot; si++)
        if (c.s.e->fileIqBlockBytes(si) < (size_t)blk * c.sflen * rows * sizeof(cf32)) throw std::runtime_error("stream: block buffer");
      c.front.tb.rotation(c.s.offset_freq_hz, c.sflen, 15000.0 * (double)c.s.e->symbolSz());   // the -o rotation of the cell's output samples, the file source's
      c.front.tb.upload(c.s.plan, st_run);
      if (c.s.filt.L) {
        c.front.ft.upload(c.s.filt, st_run);
        const int rm = reserveMid(c, midSamples(c, c.s.plan.step));
        if (rm != LSN_SUCCESS) return rm;
      }
    }
    HIP_CHECK(hipStreamSynchronize(st_run));
    return LSN_SUCCESS;
  });
}

uint64_t StreamRing::midSamples(const Cell& c, u128 step) const
{
  const ResamplePlan& p = c.s.plan;
  const u128 last = p.start + (u128)((uint64_t)blk * c.sflen - 1) * step;
  return (uint64_t)(last >> 64) - (uint64_t)(p.start >> 64) + p.taps + 2;   // inputSpan's hi - lo of blk subframes, + 2
}

int StreamRing::reserveMid(Cell& c, uint64_t samples)
{
  // called from setup() and, in front of the first push, from track(): nothing of this stream's has been launched on the buffer yet, so it may still move
  c.s.e->holdChanBuffer(false);
  const int r = c.s.e->reserveChanBuffer((size_t)samples * nant * sizeof(cf32));
  c.front.mid = c.s.e->chanBuffer();
  c.front.mid_cap = c.s.e->chanBufferSamples(nant);   // what the Phy holds now.  0: the old buffer went and no new one came - every later launch of this cell throws in front of stage 1
  if (c.front.mid) c.s.e->holdChanBuffer(true);       // from here on nobody grows - frees - it under this stream
  return r;
}

int64_t StreamRing::oldestNeeded() const
{
  if (tracking) {   // the first input sample of the next subframe to resample, at the position the loop has decided (the end of the last decided segment is one)
    int64_t oldest = (int64_t)pushed;
    for (const auto& c : cells) {
      if (c.s.max_subframes && c.filled >= c.s.max_subframes) continue;
      // (a cell with re-acquisition keeps acq_keep samples more: the span of a search of the segment behind, and room for a backward jump)
      const int64_t lo = (int64_t)(uint64_t)(c.tk.position(c.filled) >> 64) - (int64_t)c.s.plan.taps / 2 + 1 - (int64_t)c.s.filt.L - (int64_t)c.acq_keep;
      oldest = std::min(oldest, std::max<int64_t>(lo, 0));
    }
    return oldest;
  }
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
  if (tracking) return runReadyTracked(flush_all);
  for (;;) {
    if (failed != LSN_SUCCESS) return failed;
    uint32_t nsf[kFileMaxCells] = {};
    int64_t lo[kFileMaxCells] = {}, hi[kFileMaxCells] = {};
    bool any = false;
    for (size_t c = 0; c < cells.size(); c++) {
      nsf[c] = stream_cell_ready(plans[c], pushed, cells[c].done, blk, flush_all);
      if (!nsf[c]) continue;
      cells[c].s.plan.inputSpan(cells[c].done * cells[c].sflen, (uint64_t)nsf[c] * cells[c].sflen, lo[c], hi[c]);
      any = true;
    }
    if (!any) return LSN_SUCCESS;
    LsnResampleCell k[kFileMaxCells];
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      k[c] = LsnResampleCell();
      if (nsf[c]) k[c] = q.s.plan.cell(q.done * q.sflen, q.sflen, q.front.tb, bufferFor(q), (uint64_t)nsf[c] * q.sflen);
    }
    launchRing(k, lo, hi, "stream: a block");
    for (size_t c = 0; c < cells.size() && failed == LSN_SUCCESS; c++)
      if (nsf[c]) submitBlock(cells[c], nsf[c]);
  }
}

void StreamRing::launchRing(const LsnResampleCell* k, const int64_t* lo, const int64_t* hi, const char* what)
{
  // what the launch reads of the ring: the union of the cells' spans, each widened by its filter's L (0: none)
  int64_t in_lo = 0, in_hi = 0;
  bool any = false;
  for (size_t c = 0; c < cells.size(); c++) {
    if (!k[c].n_out) continue;
    const int64_t L = (int64_t)cells[c].s.filt.L;
    in_lo = any ? std::min(in_lo, lo[c] - L) : lo[c] - L;
    in_hi = any ? std::max(in_hi, hi[c] + L) : hi[c] + L;
    any = true;
  }
  in_lo = std::max<int64_t>(in_lo, 0);   // zeros in front of the stream are the kernel's
  if (in_hi > (int64_t)pushed || (uint64_t)(in_hi - in_lo) > ring_samples || (int64_t)pushed - in_lo > (int64_t)ring_samples)
    throw std::runtime_error(std::string(what) + "'s input is not in the ring");
  HIP_CHECK(hipEventRecord(ev_copy, st_copy));
  HIP_CHECK(hipStreamWaitEvent(st_run, ev_copy, 0));   // the samples pushed so far are in their slots
  const FrontCell* fc[kFileMaxCells];
  for (size_t c = 0; c < cells.size(); c++) fc[c] = &cells[c].front;
  lsn_launch_front({d_ring, fmt, sfm.scale, in_lo, (uint64_t)(in_hi - in_lo), nant, ring_samples}, fc, k, lo, hi, (uint32_t)cells.size(), st_run, what);
  Launch l;
  l.ev = takeEvent(); l.lo = in_lo;
  HIP_CHECK(hipEventRecord(l.ev, st_run));
  inflight.push_back(l);
}

cf32* StreamRing::bufferFor(Cell& q, bool empty)
{
  const int si = (int)(q.launches % (uint64_t)nslot);
  if (empty && q.mark[si]) q.s.e->waitIqConsumed(q.mark[si]);   // the block this buffer carried last has been through stage A
  return q.s.e->fileIqBlock(si);
}

void StreamRing::submitBlock(Cell& q, uint32_t nsf)
{
  closeBlock(q, nsf, tracking && q.tk.frameHolding(), tracking ? q.tk.tti(q.done) : (uint32_t)((q.s.start_tti + q.done) % 10240u));
}

void StreamRing::closeBlock(Cell& q, uint32_t nsf, bool held, uint32_t tti)
{
  const int si = (int)(q.launches % (uint64_t)nslot);
  if (held) {   // resampled and measured, not decoded: the same buffer is filled again (everything that touches it is ordered on st_run)
    q.tk.fs.held += nsf;
    q.done += nsf;
    return;
  }
  q.rc = q.s.e->submit(q.s.e->fileIqBlock(si), nsf, tti, q.s.update_meta_period, st_run);
  q.mark[si] = q.s.e->submitMark();
  q.launches++;
  q.done += nsf;
  if (q.rc != LSN_SUCCESS) failed = q.rc;   // nothing more is submitted to any Phy
}

int StreamRing::push(const void* iq, uint64_t n)
{
  if (failed != LSN_SUCCESS) return failed;
  if (n >= (1ull << 62) || pushed + n >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  const int r = guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    const uint8_t* src = (const uint8_t*)iq;
    if (tracking) {   // a gap is part of the input: a segment whose PSS subframe reads it has no measurement
      const int64_t old = oldestNeeded();
      gaps.erase(std::remove_if(gaps.begin(), gaps.end(), [old](const std::pair<int64_t, int64_t>& g) { return g.second <= old; }), gaps.end());
      if (!src && n) gaps.emplace_back((int64_t)pushed, (int64_t)(pushed + n));
    }
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
    if (tracking) for (auto& c : cells) deliver(c, 0, true);
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

// ---- the timing loop (lsn_track.h) ----

int StreamRing::track(const lsn_stream_track_cfg_t& tc, double rate_in)
{
  if (pushed || tracking || failed != LSN_SUCCESS) return LSN_ERROR_INVALID_INPUTS;
  for (const auto& c : cells) if (c.s.plan.map_nout) return LSN_ERROR_INVALID_INPUTS;   // (limit: no timing loop - and so no re-acquisition or frame sync - with an antenna map)
  TrackCfg cfg;
  const int r = track_cfg_resolve(tc.kp, tc.ki, tc.max_ppm, tc.lost_after, cfg);
  if (r != LSN_SUCCESS) return r;
  for (size_t c = 0; c < cells.size(); c++) {
    if (!std::isfinite(tc.cfo_hz[c]) || !std::isfinite(tc.initial_ppm[c]) || std::fabs(tc.initial_ppm[c]) > cfg.max_ppm) return LSN_ERROR_INVALID_INPUTS;
    if (cells[c].s.e->symbolSz() < 128) return LSN_ERROR_INVALID_INPUTS;
  }
  if ((uint64_t)trackedBlockInput(cfg.max_ppm) + 2 > ring_samples) return LSN_ERROR_INVALID_INPUTS;
  // the intermediates at the widened step: grown here, in front of the first push (nothing has been launched yet), or the call is refused
  for (auto& q : cells) {
    if (!q.s.filt.L) continue;
    const uint64_t need = midSamples(q, track_widened_step(q.s.plan.step, cfg.max_ppm));
    if (need <= q.front.mid_cap) continue;
    const int rm = reserveMid(q, need);
    if (rm != LSN_SUCCESS) return rm;
  }
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      const uint32_t N = q.s.e->symbolSz();
      if (!q.d_rep) HIP_CHECK(hipMalloc((void**)&q.d_rep, (size_t)N * sizeof(cf32)));
      if (!q.h_C) HIP_CHECK(hipHostMalloc((void**)&q.h_C, TRACK_SLOTS * kTrackLags * sizeof(float), hipHostMallocCoherent | hipHostMallocMapped));
      std::vector<double> pd(2 * (size_t)N);
      pss_replica_d(q.s.e->cellId() % 3, N, (double)tc.cfo_hz[c], pd.data());   // lsn_clock_replica's
      std::vector<cf32> rep(N);
      for (uint32_t k = 0; k < N; k++) rep[k] = {(float)pd[2 * k], (float)pd[2 * k + 1]};
      HIP_CHECK(hipMemcpy(q.d_rep, rep.data(), (size_t)N * sizeof(cf32), hipMemcpyHostToDevice));
    }
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      q.tk.init(&q.s.plan, q.sflen, q.s.e->symbolSz(), q.s.start_tti, q.s.max_subframes, rate_in, cfg, tc.enable[c] != 0, tc.initial_ppm[c]);
      q.filled = 0;
    }
    tracking = true;
    return LSN_SUCCESS;
  });
}

int64_t StreamRing::trackedBlockInput(double max_ppm) const
{
  int64_t lo = 0, hi = 0;
  for (size_t c = 0; c < cells.size(); c++) {
    const ResamplePlan& p = cells[c].s.plan;
    const int64_t half = (int64_t)p.taps / 2;
    const u128 last = p.start + (u128)((uint64_t)blk * cells[c].sflen - 1) * track_widened_step(p.step, max_ppm);
    const int64_t L = (int64_t)cells[c].s.filt.L;   // a filtered cell reads L more on both sides
    const int64_t l = (int64_t)(uint64_t)(p.start >> 64) - half + 1 - L, h = (int64_t)(uint64_t)(last >> 64) + half + 1 + L;
    lo = c ? std::min(lo, l) : l;
    hi = c ? std::max(hi, h) : h;
  }
  return hi - lo;
}

// ---- re-acquisition (lsn_track.h) ----

int StreamRing::reacquire(const lsn_stream_reacquire_cfg_t& rc)
{
  if (pushed || !tracking || reacquiring || failed != LSN_SUCCESS || filtered()) return LSN_ERROR_INVALID_INPUTS;
  if (rc.min_ratio != 0.0 && (!std::isfinite(rc.min_ratio) || rc.min_ratio < 1.0)) return LSN_ERROR_INVALID_INPUTS;
  // the ring holds what track() asked for and, behind it, the samples every searched cell keeps
  const double max_ppm = cells[0].tk.cfg.max_ppm;   // (one configuration for all cells of a stream)
  uint64_t keep[kFileMaxCells] = {}, most = 0;
  for (size_t c = 0; c < cells.size(); c++) {
    if (!rc.enable[c] || !cells[c].tk.enabled) continue;   // a cell whose loop is off has no measurement that could be lost
    keep[c] = track_acquire_keep(cells[c].s.plan.step, max_ppm, cells[c].sflen);
    most = std::max(most, keep[c]);
  }
  if ((uint64_t)trackedBlockInput(max_ppm) + 2 + most > ring_samples) return LSN_ERROR_INVALID_INPUTS;
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      if (!keep[c]) continue;
      const uint32_t N = q.s.e->symbolSz();
      if (!q.acq_x) HIP_CHECK(hipMalloc((void**)&q.acq_x, (size_t)kAcqSpanSubframes * nant * q.sflen * sizeof(cf32)));
      if (!q.acq_C) HIP_CHECK(hipHostMalloc((void**)&q.acq_C, (size_t)(kTrackSegSubframes * q.sflen / track_lag_spacing(N)) * sizeof(float), hipHostMallocCoherent | hipHostMallocMapped));
    }
    for (size_t c = 0; c < cells.size(); c++) {
      if (!keep[c]) continue;
      cells[c].acq_keep = keep[c];
      cells[c].tk.reacquire(rc.after, rc.min_ratio);
    }
    reacquiring = true;
    return LSN_SUCCESS;
  });
}

void StreamRing::launchSearches()
{
  LsnResampleCell k[kFileMaxCells];
  LsnAcquireCell a[kFileMaxCells];
  int64_t lo[kFileMaxCells] = {}, hi[kFileMaxCells] = {};
  bool any = false;
  for (size_t c = 0; c < cells.size(); c++) {
    Cell& q = cells[c];
    TrackCell& t = q.tk;
    k[c] = LsnResampleCell();
    a[c] = LsnAcquireCell();
    if (!t.search.active || t.search.launched) continue;
    t.searchInputSpan(lo[c], hi[c]);
    if (hi[c] > (int64_t)pushed) continue;   // the span is not complete yet
    t.search.launched = true;
    if (inGap(lo[c], hi[c])) continue;       // not launched: it comes back rejected (acq_ev stays null)
    k[c] = q.s.plan.cell(t.search.base, t.search.step, t.search.span, q.sflen, 0, q.front.tb, q.acq_x, (uint64_t)kAcqSpanSubframes * q.sflen);
    a[c].x = q.acq_x; a[c].rep = q.d_rep; a[c].C = q.acq_C; a[c].N = t.N; a[c].d = track_lag_spacing(t.N); a[c].sflen = q.sflen; a[c].nant = nant;
    a[c].n_lags = kTrackSegSubframes * q.sflen / a[c].d;
    any = true;
  }
  if (!any) return;
  launchRing(k, lo, hi, "stream: a search");   // a launch of its own: the scratches are no block buffers, and the decode path's launches stay what they are
  lsn_launch_pss_acquire(a, (uint32_t)cells.size(), st_run);
  for (size_t c = 0; c < cells.size(); c++) {
    if (!a[c].n_lags) continue;
    cells[c].acq_ev = takeEvent();
    HIP_CHECK(hipEventRecord(cells[c].acq_ev, st_run));
    cells[c].tk.acq_launched++;
  }
}

void StreamRing::takeSearch(Cell& q)
{
  TrackCell& t = q.tk;
  if (!t.search.active || !t.search.launched || t.search.done) return;
  if (t.nvalid + t.ninvalid < t.search.h + 2) return;   // (a status call) the measurement of segment h + 1, whose history the decision reads, is not in yet
  if (!q.acq_ev) { t.searched(nullptr); return; }
  const hipError_t e = hipEventSynchronize(q.acq_ev);
  ev_free.push_back(q.acq_ev);
  q.acq_ev = nullptr;
  HIP_CHECK(e);
  t.searched(q.acq_C);
}

int StreamRing::reacquireStatus(lsn_stream_reacquire_status_t* out)
{
  if (!out || out->struct_size != sizeof(lsn_stream_reacquire_status_t) || !reacquiring) return LSN_ERROR_INVALID_INPUTS;
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->nof_cells = (uint32_t)cells.size();
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      deliver(q, 0, true);   // the measurement of segment h + 1 comes in front of the search of segment h, as on entering h + 3
      takeSearch(q);
      const TrackCell& t = q.tk;
      out->launched[c] = t.acq_launched; out->accepted[c] = t.acq_accepted; out->rejected[c] = t.acq_rejected;
      out->last_peak[c] = t.acq_peak; out->last_ratio[c] = t.acq_ratio; out->last_offset[c] = t.acq_offset;
      out->jump_segment[c] = t.acq_jump_segment; out->jumps_total[c] = std::ldexp((double)t.acq_jumps, -64);
    }
    return LSN_SUCCESS;
  });
}

// ---- frame sync (lsn_track.h) ----

int StreamRing::frameSync(const lsn_stream_frame_sync_cfg_t& fc)
{
  if (pushed || !reacquiring || framing || failed != LSN_SUCCESS) return LSN_ERROR_INVALID_INPUTS;
  if (fc.tries > kFrameMaxTries || fc.hold > LSN_FRAME_SYNC_NO_HOLD) return LSN_ERROR_INVALID_INPUTS;
  const int r = guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      if (!fc.enable[c] || !q.tk.acq) continue;   // a cell that is never searched never jumps
      const int rm = q.s.e->reserveMibSide();
      if (rm != LSN_SUCCESS) return rm;
      if (!q.h_cand) HIP_CHECK(hipHostMalloc((void**)&q.h_cand, (size_t)TRACK_SLOTS * 4 * sizeof(LsnCand), hipHostMallocCoherent | hipHostMallocMapped));
    }
    return LSN_SUCCESS;
  });
  if (r != LSN_SUCCESS) return r;
  for (size_t c = 0; c < cells.size(); c++) {
    Cell& q = cells[c];
    if (q.h_cand && fc.enable[c]) q.tk.frameSync(fc.tries, fc.hold != LSN_FRAME_SYNC_NO_HOLD, q.s.e->nofPrb(), q.s.e->nofPorts());
  }
  framing = true;
  return LSN_SUCCESS;
}

int StreamRing::frameSyncStatus(lsn_stream_frame_sync_status_t* out)
{
  if (!out || out->struct_size != sizeof(lsn_stream_frame_sync_status_t) || !framing) return LSN_ERROR_INVALID_INPUTS;
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->nof_cells = (uint32_t)cells.size();
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      deliver(q, 0, true);   // the attempts in flight come back with their measurements; the rule looks at them when their segment's turn comes
      takeSearch(q);
      const TrackCell::Frame& f = q.tk.fs;
      out->checks[c] = f.checks; out->attempts[c] = f.attempts; out->confirmed[c] = f.confirmed; out->relabelled[c] = f.relabelled; out->given_up[c] = f.given_up;
      out->accept_segment[c] = f.accept_segment; out->relabel_segment[c] = f.relabel_segment; out->held[c] = f.held;
      out->last_sfn[c] = f.last_sfn; out->last_delta[c] = f.last_delta; out->shift[c] = f.shift;
    }
    return LSN_SUCCESS;
  });
}

bool StreamRing::inGap(int64_t lo, int64_t hi) const
{
  for (const auto& g : gaps) if (g.first < hi && lo < g.second) return true;
  return false;
}

void StreamRing::deliver(Cell& q, uint64_t upto_h, bool all)
{
  while (!q.pending.empty() && (all || q.pending.front().h <= upto_h)) {
    const Cell::Pending p = q.pending.front();
    q.pending.pop_front();
    TrackCell::Attempt at;
    at.due = p.due; at.launched = p.mib;
    if (p.ev) {
      const hipError_t e = hipEventSynchronize(p.ev);
      ev_free.push_back(p.ev);
      HIP_CHECK(e);
      if (p.mib) (void)mib_parse(q.h_cand + (size_t)p.slot * 4, at.mib);
      q.tk.measured(p.timing ? q.h_C + (size_t)p.slot * kTrackLags : nullptr, p.due ? &at : nullptr);
    } else {
      q.tk.measured(nullptr, p.due ? &at : nullptr);
    }
  }
}

// runReady of a tracked stream: every cell's block buffer fills segment by segment (or by the part of one that fits the buffer), each piece at the step its segment
// was entered with; the piece that holds a segment's first subframe is followed by the cell's window of k_pss_timing on the same stream.  One k_resample_ring launch
// carries the pieces of all cells that are due.  A buffer is submitted when blk subframes are in it (fewer: a flush, or the last ones in front of max_subframes).
int StreamRing::runReadyTracked(bool flush_all)
{
  for (;;) {
    if (failed != LSN_SUCCESS) return failed;
    LsnResampleCell k[kFileMaxCells];
    uint32_t piece[kFileMaxCells] = {};
    int64_t lo[kFileMaxCells] = {}, hi[kFileMaxCells] = {};
    bool any = false;
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      TrackCell& t = q.tk;
      k[c] = LsnResampleCell();
      if (q.s.max_subframes && q.filled >= q.s.max_subframes) continue;   // run out
      if (!t.entered || q.filled == t.segEnd()) {   // the next segment: the measurement of the segment two in front of it comes back first
        if (t.needsMeasurement()) deliver(q, t.h - 1, false);
        if (t.searchResultDue()) takeSearch(q);   // (re-acquisition: the search of the segment three in front comes back behind that measurement)
        const bool held = t.frameHolding();
        const uint32_t shift = t.fs.shift, tti = t.tti(q.done);
        t.enter();
        // (frame sync) the counting or the hold changes with this segment: what the buffer holds goes first - to the Phy or nowhere -, as what it was counted as
        if ((t.frameHolding() != held || t.fs.shift != shift) && q.filled > q.done) {
          closeBlock(q, (uint32_t)(q.filled - q.done), held, tti);
          if (failed != LSN_SUCCESS) return failed;
        }
      }
      const uint64_t end = std::min<uint64_t>(t.segEnd(), q.done + blk);
      const uint64_t upto = std::min<uint64_t>(t.completeInSegment(insideEnd(q)), end);
      if (upto <= q.filled || (upto < end && !flush_all)) continue;
      piece[c] = (uint32_t)(upto - q.filled);
      k[c] = q.s.plan.cell(t.position(q.filled), t.step, t.span, q.sflen, (uint32_t)(q.filled - q.done) * q.sflen, q.front.tb, bufferFor(q, q.filled == q.done),
                           (uint64_t)piece[c] * q.sflen);
      t.inputSpan(q.filled, upto, lo[c], hi[c]);
      any = true;
    }
    if (any) {
      launchRing(k, lo, hi, "stream: a segment");
      // the windows of the segments that began in this launch
      LsnTimingCell tm[kFileMaxCells];
      bool timing = false, mibs = false;
      const cf32* mib_sf[kFileMaxCells] = {};
      for (size_t c = 0; c < cells.size(); c++) {
        Cell& q = cells[c];
        TrackCell& t = q.tk;
        tm[c] = LsnTimingCell();
        if (!piece[c] || q.filled != t.sf0) continue;
        int64_t g_lo, g_hi;
        t.inputSpan(t.sf0, t.sf0 + 1, g_lo, g_hi);
        q.s.filt.widen(g_lo, g_hi);   // (L = 0: as it is)
        const bool gap = inGap(g_lo, g_hi);
        Cell::Pending p = {t.h, nullptr, (uint32_t)(t.h % TRACK_SLOTS), false, framing && t.frameAttemptDue(), false};
        if (p.due && !gap) {   // (frame sync) the attempt of this segment: the PBCH decode of the subframe the window looks at
          p.mib = true;
          p.ev = takeEvent();
          mibs = true;
          t.fs.attempts++;
        }
        if (t.enabled && t.hasPss() && !gap) {
          p.timing = true;
          tm[c].x = k[c].out; tm[c].rep = q.d_rep; tm[c].C = q.h_C + (size_t)p.slot * kTrackLags; tm[c].N = t.N; tm[c].d = track_lag_spacing(t.N); tm[c].sflen = q.sflen; tm[c].nant = nant;
          tm[c].n_occ = 1; tm[c].sf[0] = (uint32_t)(q.filled - q.done); tm[c].p[0] = track_pss_index(t.N);
          if (!p.ev) p.ev = takeEvent();
          timing = true;
        }
        mib_sf[c] = p.mib ? k[c].out + (size_t)(q.filled - q.done) * nant * q.sflen : nullptr;
        q.pending.push_back(p);
      }
      if (timing) {
        lsn_launch_pss_timing(tm, (uint32_t)cells.size(), st_run);
        for (size_t c = 0; c < cells.size(); c++)
          if (tm[c].n_occ && !mib_sf[c]) HIP_CHECK(hipEventRecord(cells[c].pending.back().ev, st_run));
      }
      if (mibs) {   // directly behind the windows; a cell's event lies behind its candidates' copy
        for (size_t c = 0; c < cells.size(); c++) {
          if (!mib_sf[c]) continue;
          const Cell::Pending& p = cells[c].pending.back();
          cells[c].s.e->mibLaunchSide(mib_sf[c], cells[c].h_cand + (size_t)p.slot * 4, st_run);
          HIP_CHECK(hipEventRecord(p.ev, st_run));
        }
      }
      for (size_t c = 0; c < cells.size(); c++) cells[c].filled += piece[c];
    }
    if (reacquiring) launchSearches();
    bool submitted = false;
    for (size_t c = 0; c < cells.size() && failed == LSN_SUCCESS; c++) {
      Cell& q = cells[c];
      const uint32_t n = (uint32_t)(q.filled - q.done);
      if (!n || !(n == blk || (!any && flush_all) || (q.s.max_subframes && q.filled == q.s.max_subframes))) continue;
      submitBlock(q, n);
      submitted = true;
    }
    if (!any && !submitted) return LSN_SUCCESS;
  }
}

int StreamRing::trackStatus(lsn_stream_track_status_t* out)
{
  if (!out || out->struct_size != sizeof(lsn_stream_track_status_t) || !tracking) return LSN_ERROR_INVALID_INPUTS;
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(device));
    memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->nof_cells = (uint32_t)cells.size();
    for (size_t c = 0; c < cells.size(); c++) {
      Cell& q = cells[c];
      deliver(q, 0, true);
      const TrackCell& t = q.tk;
      const double seglen = (double)(kTrackSegSubframes * q.sflen);
      out->segments[c] = t.entered ? t.h + 1 : 0;
      out->valid[c] = t.nvalid; out->invalid[c] = t.ninvalid; out->lost[c] = t.loop.lost; out->last_error[c] = t.last_e;
      out->correction_ppm[c] = t.loop.corr / seglen * 1e6; out->integrator_ppm[c] = t.loop.integ / seglen * 1e6;
      out->position_drift[c] = t.positionDrift(q.filled);
    }
    return LSN_SUCCESS;
  });
}

}  // namespace lsn

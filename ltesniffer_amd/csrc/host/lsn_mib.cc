// lsn_mib.cc - PBCH / MIB decode of one subframe 0 (srsran_ue_mib_decode + srsran_pbch_mib_unpack in the DECODE_MIB state of
// the reference, /root/reference/src/src/LTESniffer_Core.cc:382-395): the stream's SFN = MIB SFN + position of the radio frame
// in the 40 ms BCH period.  Runs the worker's own OFDM + CRS estimate (k_ofdm, k_chest, k_chest_fin) on the subframe and then
// k_pbch_llr + k_pbch_viterbi (stage_a.hip); the four candidates come back as four (bits, CRC mask) pairs.
// Three parts, shared by everyone who decodes a MIB: the launch sequence over a set of buffers on a stream (mibLaunch), the copy of the candidates to the host
// (mibFetch), and the host parse (mib_parse, HIP-free: lsn_track.cc).  mibDecode runs them on chunk slot 0 and refuses while blocks are in flight; the side decode
// (mibDecodeSide, and mibLaunchSide for a stream's frame sync: DESIGN 3.1m) runs them on a one-subframe scratch of its own, beside the pipeline.
// Product code: no CPU fallback, nothing from oracle/ is included or linked.
#include "lsn_engine.h"
#include "lsn_track.h"
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace lsn {

void Engine::mibLaunch(const cf32* d_iq, const MibBufs& b, hipStream_t st)
{
  b.h_sfidx[0] = 0;
  HIP_CHECK(hipMemcpyAsync(b.d_sfidx, b.h_sfidx, sizeof(uint32_t), hipMemcpyHostToDevice, st));
  lsn_launch_ofdm(cd, d_iq, nullptr, b.d_grid, 1, st);
  lsn_launch_chest(cd, b.d_grid, b.d_sfidx, b.d_ce, b.d_chest_raw, 1, st);
  lsn_launch_chest_fin(cd, b.d_chest_raw, b.d_chest, 1, st);
  lsn_launch_pbch(cd, b.d_grid, b.d_ce, b.d_chest, b.d_llr, b.d_cand, st);
}

void Engine::mibFetch(const MibBufs& b, LsnCand* cand4, float* llr_raw480, hipStream_t st)
{
  HIP_CHECK(hipMemcpyAsync(cand4, b.d_cand, 4 * sizeof(LsnCand), hipMemcpyDeviceToHost, st));
  if (llr_raw480) HIP_CHECK(hipMemcpyAsync(llr_raw480, b.d_llr, 480 * sizeof(float), hipMemcpyDeviceToHost, st));
}

// iq: one subframe [iq_nant][15 N] cf32; returns 1 (found), 0 (no MIB in this subframe) or a negative error
int Engine::mibDecode(const void* iq, bool on_device, lsn_mib_t* out, float* llr_raw480)
{
  if (!cell_set) return LSN_ERROR;
  if (!iq || !out) return LSN_ERROR_INVALID_INPUTS;
  if (batch_open) return LSN_ERROR;  // borrows a chunk slot: not while submitted blocks are in flight (call lsn_phy_wait first)
  std::memset(out, 0, sizeof(*out));
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(cfg.device));
    Chunk& ch = chunks[0];  // idle between process calls
    hipStream_t st = stream_a[0];
    const size_t sf_bytes = (size_t)cd.iq_nant * cd.sflen * sizeof(cf32);
    if (!mib_d_iq) {
      HIP_CHECK(hipMalloc((void**)&mib_d_iq, sf_bytes));
      HIP_CHECK(hipMalloc((void**)&mib_d_llr, 5 * 480 * sizeof(float)));
      HIP_CHECK(hipMalloc((void**)&mib_d_cand, 4 * sizeof(LsnCand)));
    }
    const cf32* d_iq = (const cf32*)iq;
    if (!on_device) {
      HIP_CHECK(hipMemcpyAsync(mib_d_iq, iq, sf_bytes, hipMemcpyHostToDevice, st));
      d_iq = mib_d_iq;
    }
    MibBufs b;
    b.d_grid = ch.d_grid; b.d_ce = ch.d_ce; b.d_chest_raw = ch.d_chest_raw; b.d_chest = ch.d_chest; b.d_sfidx = ch.d_sfidx; b.h_sfidx = ch.h_sfidx;
    b.d_llr = mib_d_llr; b.d_cand = mib_d_cand;
    mibLaunch(d_iq, b, st);
    LsnCand cand[4];
    mibFetch(b, cand, llr_raw480, st);
    HIP_CHECK(hipStreamSynchronize(st));
    return mib_parse(cand, *out) ? 1 : 0;
  });
}

// the side scratch: what allocChunk gives a slot for ONE subframe (zeroed, as there), the PBCH kernels' outputs, a staging subframe for host input, a pinned
// result slot and a stream.  Lives until the cell is set again or the engine goes (freeDevice)
void Engine::ensureMibSide()
{
  MibSide& s = mib_side;
  if (s.st) return;
  freeMibSide();   // (what an earlier call that failed half way left)
  const size_t A = dlRx(), P = cell.nof_ports;
  auto dz = [](auto*& p, size_t n) {
    HIP_CHECK(hipMalloc((void**)&p, n * sizeof(*p) + 16));
    HIP_CHECK(hipMemset(p, 0, n * sizeof(*p)));
  };
  dz(s.b.d_grid, A * 14 * cd.nre);
  dz(s.b.d_ce, P * A * 14 * cd.nre);
  dz(s.b.d_chest_raw, A * P * 8);
  dz(s.b.d_chest, 1);
  dz(s.b.d_sfidx, 1);
  dz(s.b.d_llr, 5 * 480);
  dz(s.b.d_cand, 4);
  dz(s.d_iq, (size_t)cd.iq_nant * cd.sflen);
  HIP_CHECK(hipHostMalloc((void**)&s.b.h_sfidx, 16, hipHostMallocCoherent | hipHostMallocMapped));
  HIP_CHECK(hipHostMalloc((void**)&s.h_cand, 4 * sizeof(LsnCand), hipHostMallocCoherent | hipHostMallocMapped));
  HIP_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  HIP_CHECK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));   // last: its presence says the scratch is whole
}

void Engine::freeMibSide()
{
  MibSide& s = mib_side;
  auto df = [](auto*& p) { if (p) (void)hipFree(p); p = nullptr; };
  if (s.st) { (void)hipStreamSynchronize(s.st); (void)hipStreamDestroy(s.st); s.st = nullptr; }
  if (s.ev) { (void)hipEventDestroy(s.ev); s.ev = nullptr; }
  df(s.b.d_grid); df(s.b.d_ce); df(s.b.d_chest_raw); df(s.b.d_chest); df(s.b.d_sfidx); df(s.b.d_llr); df(s.b.d_cand); df(s.d_iq);
  if (s.b.h_sfidx) { (void)hipHostFree(s.b.h_sfidx); s.b.h_sfidx = nullptr; }
  if (s.h_cand) { (void)hipHostFree(s.h_cand); s.h_cand = nullptr; }
  s.queued = false;
}

int Engine::mibDecodeSide(const void* iq, bool on_device, lsn_mib_t* out, float* llr_raw480)
{
  if (!cell_set) return LSN_ERROR;
  if (!iq || !out) return LSN_ERROR_INVALID_INPUTS;
  std::memset(out, 0, sizeof(*out));
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> lk(mib_side.mtx);
    HIP_CHECK(hipSetDevice(cfg.device));
    ensureMibSide();
    MibSide& s = mib_side;
    if (s.queued) HIP_CHECK(hipStreamWaitEvent(s.st, s.ev, 0));   // a stream's decode may still run in the scratch
    const cf32* d_iq = (const cf32*)iq;
    if (!on_device) {
      HIP_CHECK(hipMemcpyAsync(s.d_iq, iq, (size_t)cd.iq_nant * cd.sflen * sizeof(cf32), hipMemcpyHostToDevice, s.st));
      d_iq = s.d_iq;
    }
    mibLaunch(d_iq, s.b, s.st);
    mibFetch(s.b, s.h_cand, llr_raw480, s.st);
    HIP_CHECK(hipStreamSynchronize(s.st));
    return mib_parse(s.h_cand, *out) ? 1 : 0;
  });
}

int Engine::reserveMibSide()
{
  if (!cell_set) return LSN_ERROR;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> lk(mib_side.mtx);
    HIP_CHECK(hipSetDevice(cfg.device));
    ensureMibSide();
    return LSN_SUCCESS;
  });
}

void Engine::mibLaunchSide(const cf32* d_iq, LsnCand* h_cand4, hipStream_t st)
{
  std::lock_guard<std::mutex> lk(mib_side.mtx);   // (a mibDecodeSide of the caller's has returned, so the scratch is idle or belongs to `st`)
  MibSide& s = mib_side;
  if (!s.st) throw std::runtime_error("mib: the side scratch was not reserved");
  mibLaunch(d_iq, s.b, st);
  mibFetch(s.b, h_cand4, nullptr, st);
  HIP_CHECK(hipEventRecord(s.ev, st));
  s.queued = true;
}

}  // namespace lsn

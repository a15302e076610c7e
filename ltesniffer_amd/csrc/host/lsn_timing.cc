// lsn_timing.cc - lsn_pss_timing and lsn_pss_acquire: k_pss_timing and k_pss_acquire (kernels/track.hip) without a Phy, the siblings of lsn_clock_track (DESIGN.md
// sections 3.1h and 3.1k).  The stream's own use of the kernels is in lsn_stream_ring.cc.  Product code: no CPU fallback for the correlation.
#include "lsn_hip.h"
#include "../kernels/lsn_dev.h"
#include "lsn_track.h"
#include "lsn_track_launch.h"
#include <algorithm>
#include <vector>

namespace {

struct DevMem {
  void* p = nullptr;
  ~DevMem() { if (p) (void)hipFree(p); }
  void alloc(size_t bytes) { HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 8))); }
};

}  // namespace

// k_pss_acquire without a Phy: all cells in one launch
extern "C" int lsn_pss_acquire(int device, int blocks_on_device, const lsn_pss_acquire_cell_t* cells, uint32_t n_cells)
{
  return lsn::guarded([&]() -> int {
    if (!cells || !n_cells || n_cells > LSN_TIMING_MAX_CELLS) return LSN_ERROR_INVALID_INPUTS;
    for (uint32_t c = 0; c < n_cells; c++) {   // refused before a device is touched
      const lsn_pss_acquire_cell_t& k = cells[c];
      if (k.struct_size != sizeof(lsn_pss_acquire_cell_t) || k.N < 128 || k.N > 2048 || k.d != lsn::track_lag_spacing(k.N) || k.sflen != 15 * k.N || k.nof_antennas < 1 ||
          k.nof_antennas > 8 || (75 * k.N) % (k.d * LSN_ACQ_TILE) || !k.blocks || !k.replica || !k.C)
        return LSN_ERROR_INVALID_INPUTS;
    }
    if (!lsn::have_device(device)) return LSN_ERROR_NO_DEVICE;
    HIP_CHECK(hipSetDevice(device));
    lsn::OwnedStream st;
    std::vector<DevMem> mem(3 * (size_t)n_cells);
    LsnAcquireCell L[LSN_TIMING_MAX_CELLS];
    for (uint32_t c = 0; c < n_cells; c++) {
      const lsn_pss_acquire_cell_t& k = cells[c];
      LsnAcquireCell& b = L[c];
      b = LsnAcquireCell();
      const size_t xbytes = (size_t)LSN_ACQ_SUBFRAMES * k.nof_antennas * k.sflen * sizeof(cf32);
      if (blocks_on_device) {
        b.x = (const cf32*)k.blocks;
      } else {
        mem[3 * c].alloc(xbytes);
        HIP_CHECK(hipMemcpyAsync(mem[3 * c].p, k.blocks, xbytes, hipMemcpyHostToDevice, st));
        b.x = (const cf32*)mem[3 * c].p;
      }
      mem[3 * c + 1].alloc((size_t)k.N * sizeof(cf32));
      HIP_CHECK(hipMemcpyAsync(mem[3 * c + 1].p, k.replica, (size_t)k.N * sizeof(cf32), hipMemcpyHostToDevice, st));
      b.rep = (const cf32*)mem[3 * c + 1].p;
      b.N = k.N; b.d = k.d; b.sflen = k.sflen; b.nant = k.nof_antennas; b.n_lags = 75 * k.N / k.d;
      mem[3 * c + 2].alloc((size_t)b.n_lags * sizeof(float));
      b.C = (float*)mem[3 * c + 2].p;
    }
    lsn_launch_pss_acquire(L, n_cells, st);
    for (uint32_t c = 0; c < n_cells; c++) HIP_CHECK(hipMemcpyAsync(cells[c].C, L[c].C, (size_t)L[c].n_lags * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return LSN_SUCCESS;
  });
}

extern "C" int lsn_pss_timing(int device, int blocks_on_device, const lsn_pss_timing_cell_t* cells, uint32_t n_cells)
{
  return lsn::guarded([&]() -> int {
    if (!cells || !n_cells || n_cells > LSN_TIMING_MAX_CELLS) return LSN_ERROR_INVALID_INPUTS;
    uint32_t most = 0;
    for (uint32_t c = 0; c < n_cells; c++) {   // refused before a device is touched
      const lsn_pss_timing_cell_t& k = cells[c];
      if (k.struct_size != sizeof(lsn_pss_timing_cell_t) || k.N < 128 || k.N > 2048 || k.d != lsn::track_lag_spacing(k.N) || !k.sflen || k.nof_antennas < 1 || k.nof_antennas > 8 ||
          !k.nof_subframes || k.nof_subframes > 65536 || k.n_occ > 65536 || !k.blocks || !k.replica || (k.n_occ && (!k.occ || !k.C)))
        return LSN_ERROR_INVALID_INPUTS;
      for (uint32_t o = 0; o < k.n_occ; o++) {
        const uint32_t sf = k.occ[2 * o], p = k.occ[2 * o + 1];
        if (sf >= k.nof_subframes || p < 6 * k.d || (uint64_t)p + 6 * k.d + k.N > k.sflen) return LSN_ERROR_INVALID_INPUTS;
      }
      most = std::max(most, k.n_occ);
    }
    if (!most) return LSN_SUCCESS;
    if (!lsn::have_device(device)) return LSN_ERROR_NO_DEVICE;
    HIP_CHECK(hipSetDevice(device));
    lsn::OwnedStream st;
    std::vector<DevMem> mem(3 * (size_t)n_cells);
    LsnTimingCell base[LSN_TIMING_MAX_CELLS];
    for (uint32_t c = 0; c < n_cells; c++) {
      const lsn_pss_timing_cell_t& k = cells[c];
      LsnTimingCell& b = base[c];
      b = LsnTimingCell();
      const size_t xbytes = (size_t)k.nof_subframes * k.nof_antennas * k.sflen * sizeof(cf32);
      if (blocks_on_device) {
        b.x = (const cf32*)k.blocks;
      } else {
        mem[3 * c].alloc(xbytes);
        HIP_CHECK(hipMemcpyAsync(mem[3 * c].p, k.blocks, xbytes, hipMemcpyHostToDevice, st));
        b.x = (const cf32*)mem[3 * c].p;
      }
      mem[3 * c + 1].alloc((size_t)k.N * sizeof(cf32));
      HIP_CHECK(hipMemcpyAsync(mem[3 * c + 1].p, k.replica, (size_t)k.N * sizeof(cf32), hipMemcpyHostToDevice, st));
      b.rep = (const cf32*)mem[3 * c + 1].p;
      mem[3 * c + 2].alloc((size_t)k.n_occ * LSN_TIMING_LAGS * sizeof(float));
      b.C = (float*)mem[3 * c + 2].p;
      b.N = k.N; b.d = k.d; b.sflen = k.sflen; b.nant = k.nof_antennas;
    }
    for (uint32_t o0 = 0; o0 < most; o0 += LSN_TIMING_MAX_OCC) {   // four occurrences of every cell per launch
      LsnTimingCell L[LSN_TIMING_MAX_CELLS];
      for (uint32_t c = 0; c < n_cells; c++) {
        L[c] = base[c];
        const uint32_t n = cells[c].n_occ > o0 ? std::min(cells[c].n_occ - o0, LSN_TIMING_MAX_OCC) : 0;
        L[c].n_occ = n;
        L[c].C = base[c].C + (size_t)o0 * LSN_TIMING_LAGS;
        for (uint32_t o = 0; o < n; o++) { L[c].sf[o] = cells[c].occ[2 * (o0 + o)]; L[c].p[o] = cells[c].occ[2 * (o0 + o) + 1]; }
      }
      lsn_launch_pss_timing(L, n_cells, st);
    }
    for (uint32_t c = 0; c < n_cells; c++)
      if (cells[c].n_occ) HIP_CHECK(hipMemcpyAsync(cells[c].C, base[c].C, (size_t)cells[c].n_occ * LSN_TIMING_LAGS * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return LSN_SUCCESS;
  });
}

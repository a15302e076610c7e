// lsn_sync_ant.h - the cell search over all receive antennas: k_pss_corr_ant's launcher (kernels/sync_ant.hip) and the search itself
// (lsn_sync_ant.cc), which the carrier scan calls on the channels of a bank.
#pragma once
#include "lsn_hip.h"

struct cf32;

// nch channels of A antennas each: antenna a of channel c at x + c x_stride + a ant_stride, its lags lag0 .. lag0 + nlag - 1 to C + c c_stride + r W5 + (n - lag0)
void lsn_launch_pss_corr_ant(const cf32* x, size_t x_stride, size_t ant_stride, uint32_t A, const cf32* p, uint32_t N, uint32_t W5, uint32_t P, uint32_t nroots, uint32_t lag0,
                             uint32_t nlag, float* C, size_t c_stride, uint32_t nch, hipStream_t s);

namespace lsn {

static constexpr uint32_t kSearchAntCap = 8;   // what the carrier scan may bring (its nof_antennas limit); the public call stops at LSN_SEARCH_MAX_ANTENNAS

// antenna a at iq + a ant_stride, nsamples each; max_ant: the caller's limit on nof_antennas (<= kSearchAntCap)
int cell_search_ant(int device, const cf32* iq, bool on_device, uint64_t nsamples, uint64_t ant_stride, uint32_t nof_antennas, uint32_t max_ant, uint32_t nof_prb, int rates,
                    const lsn_cell_search_cfg_t& cfg, lsn_cell_search_t& out, lsn_cell_search_ant_t* per_ant, float* corr_out);

}  // namespace lsn

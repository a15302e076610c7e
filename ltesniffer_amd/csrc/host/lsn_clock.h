// lsn_clock.h - the sample-clock estimate of a recording: what lsn_clock.cc shares with the rest of the host code.
#pragma once
#include <cstdint>

namespace lsn {

// lsn_sync.cc: the unit-energy time-domain PSS replica in double, (re, im) pairs, times exp(2 pi j rot_hz n / (15 kHz N)) when rot_hz != 0
void pss_replica_d(uint32_t n_id_2, uint32_t N, double rot_hz, double* p);

static constexpr uint32_t kClockGuard = 4;          // g: lags on either side of every window beyond what the drift asks for
static constexpr uint32_t kClockRound0 = 8;         // periods of round 0; every later round takes four times as many
static constexpr uint32_t kClockMaxPeriods = 4096;  // max_periods = 0

}  // namespace lsn

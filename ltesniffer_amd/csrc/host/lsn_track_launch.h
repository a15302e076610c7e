// lsn_track_launch.h - the launchers of kernels/track.hip (k_pss_timing, k_pss_acquire): the part of the timing loop's host side that speaks the HIP runtime's types (lsn_track.h,
// the loop and the segments, does not).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct cf32;

#define LSN_TIMING_LAGS 13u       // l_j = (j - 6) d, j = 0 .. 12
#define LSN_TIMING_MAX_CELLS 8u
#define LSN_TIMING_MAX_OCC 4u     // occurrences of one cell in one launch: a block buffer of 16 subframes holds at most four PSS

// what one cell of a k_pss_timing launch brings: occurrence o is the window around sample p[o] of subframe sf[o] of x; its 13 values go to C[13 o ...]
struct LsnTimingCell {
  const cf32* x;      // [subframe][antenna][sflen]
  const cf32* rep;    // [N] the replica (lsn_clock_replica's)
  float* C;           // [n_occ][13]; device memory, or pinned host memory the device writes
  uint32_t N, d;      // symbol size; lag spacing max(1, N / 128)
  uint32_t sflen, nant;
  uint32_t n_occ;     // 0: the cell takes no part in this launch
  uint32_t sf[LSN_TIMING_MAX_OCC], p[LSN_TIMING_MAX_OCC];   // [p - 6 d, p + 6 d + N) lies inside the subframe
  uint32_t pad;
};
void lsn_launch_pss_timing(const LsnTimingCell* cells, uint32_t n_cells, hipStream_t s);

#define LSN_ACQ_TILE 16u          // consecutive lags one workgroup of k_pss_acquire takes
#define LSN_ACQ_SUBFRAMES 6u      // the span of a search: a half frame of lags and one window more

// what one cell of a k_pss_acquire launch brings: the span x of 6 subframes - 90 N samples per antenna, contiguous in time - and the 75 N / d lags L_i = i d from its
// first sample on; value i goes to C[i]
struct LsnAcquireCell {
  const cf32* x;      // [6][antenna][sflen], sflen = 15 N
  const cf32* rep;    // [N]
  float* C;           // [75 N / d]; device memory, or pinned host memory the device writes
  uint32_t N, d;      // symbol size; lag spacing max(1, N / 128)
  uint32_t sflen, nant;
  uint32_t n_lags;    // 75 N / d, a multiple of LSN_ACQ_TILE; 0: the cell takes no part in this launch
  uint32_t pad;
};
void lsn_launch_pss_acquire(const LsnAcquireCell* cells, uint32_t n_cells, hipStream_t s);

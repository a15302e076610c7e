// lsn_front_source.h - the buffer a front-end launch reads (resampler, channel filter, channel bank) and the two rules every path to such a launch checks it by:
// the ring rule and "the input holds what these outputs read".  HIP-free integer arithmetic: it runs - and is tested (tests/native/test_front_source.cc) - on a
// machine with no GPU.
#pragma once
#include <stdint.h>

// what a launch reads: [sample][antenna] in format fmt, element 0 = sample buf_base (>= 0) of the recording, buf_len samples per antenna; what a kernel reads outside
// of [buf_base, buf_base + buf_len) (and in front of sample 0) reads as zeros.  ring_samples != 0: raw is a device ring of that many samples per antenna, sample n of
// the recording at slot n & (ring_samples - 1), [buf_base, buf_base + buf_len) are the recording indices whose samples the ring holds, and lsn_ring_holds(ring_samples,
// buf_len)
struct LsnFrontSource {
  const void* raw; uint32_t fmt; float scale;
  int64_t buf_base; uint64_t buf_len;
  uint32_t nant;
  uint64_t ring_samples;   // 0: a linear buffer
};

// the ring rule: a power of two of at most 2^32 samples (the kernels' ring_mask has 32 bits) that holds a window of `window` samples
inline bool lsn_ring_holds(uint64_t ring_samples, uint64_t window)
{
  return ring_samples && !(ring_samples & (ring_samples - 1)) && ring_samples <= (1ull << 32) && window <= ring_samples;
}

// does the window [in_base, in_base + n_in) of recording indices hold what outputs that read [lo, hi) need?  What lies in front of sample 0 reads as zeros and
// needs no sample: .lo = max(lo, 0), .len = the samples from need_lo up to hi (0 when there are none) - both formed whatever the verdict.  in_base, n_in < 2^62
struct LsnWindowNeed { bool ok; int64_t lo; uint64_t len; };
inline LsnWindowNeed lsn_window_holds(uint64_t in_base, uint64_t n_in, int64_t lo, int64_t hi)
{
  const int64_t need_lo = lo > 0 ? lo : 0;
  return {need_lo >= (int64_t)in_base && hi <= (int64_t)(in_base + n_in), need_lo, hi > need_lo ? (uint64_t)(hi - need_lo) : 0};
}

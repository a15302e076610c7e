// lsn_fft_map.h - who computes what, and where it lies, in the symbol transform of lsn_dsp.h (k_ofdm, k_ul_fft); usable on host and device.
// The transform is the oracle's radix-2 decimation in time over a work array v[0 .. M) that starts as v[brev(n)] = x[n]; stage q pairs v[i], v[i + 2^q].
// A PASS runs R consecutive stages on groups of 2^R elements held in registers.  Pass 0 is always radix 8 and takes its operands straight from the time
// samples; the passes in between exchange v through LDS; the last pass of a power-of-two size hands its registers to the carrier map.  N = 3 M (384, 768,
// 1536) runs three M-point transforms (blocks r = 0, 1, 2 of x[3 m + r]) side by side and combines them from LDS.  256 threads.
// This header is the only copy of the rule: lsn_symbol_fft indexes with it and tests/native/test_fft_schedule.cc replays the schedule and counts the LDS
// bank conflicts with it.
#pragma once
#include <stdint.h>
#ifndef LSN_HD
#ifdef __HIPCC__
#define LSN_HD __host__ __device__ __forceinline__
#else
#define LSN_HD static inline
#endif
#endif

#define LSN_FFT_THREADS 256

// log2 of the radix of the pass that starts with `s` stages done: 8 first, then 8 while three stages are left, then 4 or 2
LSN_HD int lsn_fft_radix(int lgM, int s) { return (s == 0 || lgM - s >= 3) ? 3 : lgM - s; }

// -------- pass 0: thread t < N / 8 loads time samples t + (N / 8) jj, jj = 0 .. 7 (coalesced across t).  They are x_r[tt + (M / 8) jj] of block r = t % nb
// with tt = t / nb, i.e. the operands of group g = brev(tt) of that block: register j of the group (element 8 g + j of v) is load number brev3(j).
LSN_HD int lsn_fft_first_sample(int t, int jj, int N) { return t + (N >> 3) * jj; }
LSN_HD int lsn_fft_brev3(int j) { return ((j & 1) << 2) | (j & 2) | ((j >> 2) & 1); }
LSN_HD void lsn_fft_first_group(int t, int nb, int lgM, int* r, int* g)
{
  const int tt = nb == 3 ? t / 3 : t;
  *r = nb == 3 ? t - 3 * tt : 0;
#if defined(__has_builtin) && __has_builtin(__builtin_bitreverse32)
  *g = (int)(__builtin_bitreverse32((uint32_t)tt) >> (35 - lgM));
#else
  int b = 0;
  for (int k = 0; k < lgM - 3; k++) b |= ((tt >> k) & 1) << (lgM - 4 - k);
  *g = b;
#endif
}

// -------- later passes (s stages done, radix 2^R): the nb (M >> R) groups are numbered G = r (M >> R) + g and thread t takes G = t + 256 u, u = 0, 1, ...
// Group g holds v[base + j 2^s], j < 2^R.  In the last pass base = g, so for fixed (u, j) consecutive threads hold consecutive bins.
LSN_HD int lsn_fft_groups(int nb, int lgM, int R) { return nb << (lgM - R); }
LSN_HD int lsn_fft_base(int g, int s, int R) { return ((g >> s) << (s + R)) | (g & ((1 << s) - 1)); }
// index into the table exp(-2 pi i k / M), k < M / 2, of the butterfly of stage `stage` whose upper element has offset pos < 2^stage inside its span
LSN_HD int lsn_fft_twiddle(int pos, int stage, int lgM) { return pos << (lgM - stage - 1); }

// -------- storage: element i of block r lies at cf32 slot lsn_fft_store(r, i, lgM) of the LDS image (nb M slots, no padding).  lsn_fft_slot permutes the 32
// slots of a 256-byte row by bits of the row number.  It is linear over GF(2): slot(a | b) = slot(a) ^ slot(b) for disjoint a, b, so the eight elements
// of a group are lsn_fft_store(r, base) ^ lsn_fft_slot(j << s).  With it every 8-byte read of a pass is conflict-free within 32 lanes (64 banks) and every
// 8-byte write at most 2-way within 16 lanes (32 banks) (none at 512, 1024, 2048); the block constants keep the three blocks of N = 3 M apart.
LSN_HD int lsn_fft_slot(int i) { return i ^ ((i >> 3) & 0x1C) ^ ((i >> 5) & 2) ^ ((i >> 7) & 0xF); }
LSN_HD int lsn_fft_block_key(int r) { return (0x1A20 >> (5 * r)) & 31; }  // 0, 17, 6
LSN_HD int lsn_fft_store(int r, int i, int lgM) { return (r << lgM) | (lsn_fft_slot(i) ^ lsn_fft_block_key(r)); }
LSN_HD int lsn_fft_lds_slots(int N) { return N; }

// -------- carriers: bin -> row index k of the nre kept carriers (N - nre / 2 ..., then dc ... dc + nre / 2 - 1), or -1
LSN_HD int lsn_fft_carrier(int bin, int N, int nre, int dc)
{
  const int hf = nre >> 1;
  if (bin >= N - hf) return bin - (N - hf);
  if (bin >= dc && bin < dc + hf) return bin - dc + hf;
  return -1;
}
LSN_HD int lsn_fft_carrier_bin(int k, int N, int nre, int dc) { return k < (nre >> 1) ? N - (nre >> 1) + k : k - (nre >> 1) + dc; }
// bin of a power-of-two size -> its place in the last pass (radix 2^R, s = lgM - R): thread, group number u of that thread, register j
LSN_HD void lsn_fft_last_owner(int bin, int lgM, int R, int* t, int* u, int* j)
{
  const int g = bin & ((1 << (lgM - R)) - 1);
  *j = bin >> (lgM - R);
  *t = g & (LSN_FFT_THREADS - 1);
  *u = g >> 8;
}

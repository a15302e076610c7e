// lsn_types.h - plain data shared by the HIP kernels, the host engine and the HIP-free host logic (no HIP includes).
#pragma once
#include <stdint.h>

#define LSN_MAX_LOC 160       // falcon_ue_dl.h:39 MAX_CANDIDATES_BLIND
#define LSN_MAX_SIZES 8       // distinct DCI payload sizes per cell
#define LSN_MAX_NUM_OF_CCE 84 // falcon_pdcch.h:36
#define LSN_CCE_STRIDE 96

// one blind-decode result: (location, DCI size) of one subframe
struct LsnCand {
  unsigned long long bits;  // payload bit i at position 63-i
  uint32_t rnti;            // CRC remainder = RNTI (falcon_pdcch.c:399-402)
  uint32_t flags;           // bit 0: decoded (0 = skipped: location out of range / insufficient power / all-zero LLRs);
                            // bits 1-2: search-space verdict of (location, rnti): 0 invalid, 1 ambiguous with L-1, 2 valid;
                            // LSN_CAND_NOT_COMPUTED: the slot was left out (an ancestor location holds a candidate the search was predicted to accept) -
                            // a search that comes here all the same has it decoded on demand
};
#define LSN_CAND_NOT_COMPUTED 0x80u
// The sequential search decides on RNTI, search-space verdict and the first payload bit (format 0 or 1A); the payload itself is only wanted of the dozen DCIs
// it accepts.  Its view of a slot is therefore one word - 5 KB per subframe to pull into the search thread's cache instead of 20 (that thread bounds a cell, and a
// third of its time was waiting for the table): bits 0-15 the CRC remainder, 16 decoded, 17-18 the verdict, 19 payload bit 0, 23 LSN_CAND_NOT_COMPUTED
#define LSN_CAND_HOT(bits, rnti, flags) (((uint32_t)(rnti) & 0xFFFFu) | (((uint32_t)(flags) & 0x87u) << 16) | ((uint32_t)((unsigned long long)(bits) >> 63) << 19))
// Candidate pruning (k_viterbi, stage_a.hip): the stateless part of the prediction - the RNTI manager's format table as the kernel needs it.  Format f =
// index in falcon_ue_all_formats = the RNTI manager's format index = DciFormat.  Intervals: first | last << 16, at most four per format and kind (more: pruning off).
// The stateful part (active RNTIs as 2048 words of bits, then the primary-format mask) travels per chunk: LSN_PRUNE_SNAP_WORDS words.
struct LsnPruneCfg {
  uint32_t on;             // 0: exhaustive table (every slot decoded, as rounds 1-5)
  uint32_t fmt_size[9];    // size index of format f
  uint32_t n_ever[9], n_forb[9];
  uint32_t ever[9][4], forb[9][4];
};
#define LSN_PRUNE_SNAP_WORDS 2052

// one turbo code block
struct LsnCbDev {
  uint32_t e_off;     // int16 element offset of this code block's rate-matched LLRs
  uint32_t E;
  uint32_t K, F, rv;
  uint32_t crc_b;     // 1: CRC24B (C>1), 0: CRC24A
  uint32_t out_off;   // byte offset in the payload arena
  uint32_t out_bytes; // (K - F - 24*crc_b)/8
  uint32_t il_off;    // word offset of this block size's table in LsnCellDev::turbo_il (turbo_il_offset(K))
  uint32_t reserved;
  uint32_t max_iter;
  uint32_t res_idx;   // slot of this block's LsnCbRes (launch order is sorted by size, results are not)
  uint32_t dep;       // res_idx of the FIRST code block of the same transport block when this one may be skipped once that one has failed
                      // (a transport block fails as soon as any of its code blocks fails); 0xFFFFFFFF: always decode
  uint32_t spp_off;   // u32 word offset (multiple of 4) of the block's de-rate-matched soft data: K packed words + 12 termination values (k_rm -> k_turbo)
  uint32_t nwin;      // lsn_turbo_nwin(K), from the host's table (0: the kernel works it out itself)
};
#define LSN_SPP_WORDS(K) (((K) + 12u + 3u) & ~3u)
#define LSN_CB_NODEP 0xFFFFFFFFu   // LsnCbDev::dep: always decode
// largest code block two of which share one decoder workgroup (one wavefront and half of the LDS slot each): 2 x (6 K + 16 + 3584) <= 40 960 = a quarter of the CU's LDS
#define LSN_TURBO_PAIR_KMAX 2752u
struct LsnCbRes { uint32_t ok, iters, rem_a, iters_run; uint32_t cyc_rm, cyc_map, cyc_out, cyc_all; };  // cyc_*: shader cycles per phase (s_memtime)

// ---- ingest (host only, HIP-free)
// The sample-format rule of every entry that takes IQ samples (lsn_phy_process_host[_int], lsn_phy_process_file[_rate], lsn_resample[_span]):
// (format, caller's scale) -> valid?, bytes of one complex sample, the scale the conversion multiplies with.  cf32 is taken as it is (its scale
// field is not looked at); integer samples want a finite scale >= 0, 0 = the default of full scale -> 1.0.  LSN_FMT_* = LSN_FILE_* of the public header.
enum : uint32_t { LSN_FMT_CF32 = 0, LSN_FMT_SC16 = 1, LSN_FMT_SC8 = 2 };
struct LsnSampleFormat { bool valid; uint32_t bytes; float scale; };
inline LsnSampleFormat lsn_sample_format(uint32_t fmt, float scale)
{
  if (fmt == LSN_FMT_CF32) return {true, 8u, 1.0f};
  if (fmt > LSN_FMT_SC8 || !(scale >= 0.0f && scale < __builtin_inff())) return {false, 0u, 0.0f};
  const bool sc16 = fmt == LSN_FMT_SC16;
  return {true, sc16 ? 4u : 2u, scale != 0.0f ? scale : sc16 ? 1.0f / 32768.0f : 1.0f / 128.0f};
}

// Round-robin hand-out of the blocks of a staging area that several ingest paths share.  A slot remembers the mark its last user recorded
// (Engine::submitMark: the chunks submitted so far); the next user of the slot, whichever path it comes from, waits for that mark before it
// overwrites the block.  Bookkeeping only, no lock of its own: the engine calls it under its mutex and waits outside.
struct StagingRing {
  static constexpr uint32_t MAX_SLOTS = 16;
  explicit StagingRing(uint32_t nslots) : n(nslots < 1 ? 1 : nslots > MAX_SLOTS ? MAX_SLOTS : nslots) {}
  uint32_t slots() const { return n; }
  // the next slot; wait_for: the mark to wait for in front of its reuse, 0 = never used
  uint32_t acquire(uint64_t& wait_for) { const uint32_t s = next; next = (next + 1) % n; wait_for = marks[s]; return s; }
  void retire(uint32_t slot, uint64_t mark) { marks[slot] = mark; }
private:
  const uint32_t n;
  uint32_t next = 0;
  uint64_t marks[MAX_SLOTS] = {};
};

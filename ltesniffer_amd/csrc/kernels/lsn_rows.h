// lsn_rows.h - the row geometry of the PDSCH demodulator (k_pdsch_demod, stage_c.hip), usable on host and device.
// A ROW of a decode job is one (symbol l >= l0, PRB allocated in the slot of l): twelve subcarriers.  Rows are numbered in mapping order - symbol-major,
// PRBs ascending; the PRB set may differ between the two slots (prb_mask[2]), and a subframe has 2 nslot symbols (14, or 12 with the extended CP).  A
// demodulator workgroup takes LSN_ROWS_PER_ITEM consecutive rows of one job, so a job costs ceil(rows / 16) workgroups whatever its place in the band.
// This header is the only copy of the rule: the host counts a job's work items with it, k_pdsch_prep_up lays the per-slot PRB lists out with it and
// k_pdsch_demod finds (symbol, slot, ordinal) of a row with it.
#pragma once
#include <stdint.h>
#ifndef LSN_HD
#ifdef __HIPCC__
#define LSN_HD __host__ __device__ __forceinline__
#else
#define LSN_HD static inline
#endif
#endif

#define LSN_ROWS_PER_ITEM 16u
#define LSN_ROWS_DIV_SHIFT 20   // row / n = row * div_m >> 20, exact while row * n < 2^20 (rows < 14 * 110, n <= 110) and row * div_m < 2^32

// The rows of one job.  Precondition: l0 < nslot (at most four control symbols against six or seven symbols of a slot).
struct LsnRowGeom {
  uint32_t n[2];      // allocated PRBs of slot 0 / slot 1
  uint32_t div_m[2];  // floor(2^20 / n) + 1 (n = 0: 0, the slot has no row)
  uint32_t rows0;     // rows of slot 0 = (nslot - l0) n[0]; the first row of slot 1
  uint32_t rows;      // rows0 + nslot n[1]
};

// allocated PRBs of one slot's mask below PRB `prb` (prb = nof_prb: all of them; mask bits at and above nof_prb do not count when prb <= nof_prb)
LSN_HD uint32_t lsn_rows_ordinal(const uint32_t mask[4], uint32_t prb)
{
  uint32_t n = 0;
  for (uint32_t w = 0; w < 4; w++) {
    const uint32_t lo = 32u * w;
    if (prb >= lo + 32u) n += (uint32_t)__builtin_popcount(mask[w]);
    else if (prb > lo) n += (uint32_t)__builtin_popcount(mask[w] & ((1u << (prb - lo)) - 1u));
  }
  return n;
}

LSN_HD LsnRowGeom lsn_rows_geom(const uint32_t prb_mask[2][4], uint32_t l0, uint32_t nslot, uint32_t nof_prb)
{
  LsnRowGeom g;
  for (int s = 0; s < 2; s++) {
    g.n[s] = lsn_rows_ordinal(prb_mask[s], nof_prb);
    g.div_m[s] = g.n[s] ? (1u << LSN_ROWS_DIV_SHIFT) / g.n[s] + 1u : 0u;
  }
  g.rows0 = (nslot - l0) * g.n[0];
  g.rows = g.rows0 + nslot * g.n[1];
  return g;
}

// work items (groups of LSN_ROWS_PER_ITEM rows) of a job; item i covers rows [16 i, min(16 i + 16, rows))
LSN_HD uint32_t lsn_rows_items(const LsnRowGeom& g) { return (g.rows + LSN_ROWS_PER_ITEM - 1u) / LSN_ROWS_PER_ITEM; }

// row < g.rows -> its symbol, its slot and the ordinal of its PRB among the allocated PRBs of that slot (selects, no branch: `row` is a per-lane value)
LSN_HD void lsn_rows_locate(const LsnRowGeom& g, uint32_t l0, uint32_t nslot, uint32_t row, uint32_t* l, uint32_t* slot, uint32_t* ord)
{
  const uint32_t s = row >= g.rows0 ? 1u : 0u;
  const uint32_t r = s ? row - g.rows0 : row, n = s ? g.n[1] : g.n[0], m = s ? g.div_m[1] : g.div_m[0];
  const uint32_t q = (r * m) >> LSN_ROWS_DIV_SHIFT;   // symbol inside the slot's part
  *slot = s;
  *l = (s ? nslot : l0) + q;
  *ord = r - q * n;
}

// Layout of a job's part of the prefix arena, in u16 elements from prefix_off: [14][nof_prb] REs in front of a PRB inside its symbol, [16] REs in front of
// a symbol (entry 14: all of them), then the two per-slot lists of allocated PRBs, ascending, one byte each: [2][nof_prb] bytes.
LSN_HD uint32_t lsn_rows_sym_off(uint32_t nof_prb) { return 14u * nof_prb; }
LSN_HD uint32_t lsn_rows_list_off(uint32_t nof_prb) { return 14u * nof_prb + 16u; }   // (u16 elements; the list of slot s starts s * nof_prb BYTES behind it)
LSN_HD uint32_t lsn_rows_prefix_len(uint32_t nof_prb) { return 15u * nof_prb + 16u; }

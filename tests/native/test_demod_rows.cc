// test_demod_rows.cc - the PDSCH demodulator's row geometry (ltesniffer_amd/csrc/kernels/lsn_rows.h) against a brute-force enumeration of the
// (symbol, PRB) pairs of an allocation.  The per-slot PRB lists are built the way k_pdsch_prep_up builds them (list[slot][lsn_rows_ordinal(prb)] = prb)
// and a row is resolved the way k_pdsch_demod resolves it (lsn_rows_locate, then the list).  No GPU.  One line per group of cases:
//   <name>: <cases> cases <rows> rows <errors> errors
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../ltesniffer_amd/csrc/kernels/lsn_rows.h"

struct Tally { long cases = 0, rows = 0, errors = 0; };

static void fail(Tally& t, const char* what, uint32_t nprb, uint32_t nslot, uint32_t l0, uint32_t a, uint32_t b)
{
  if (t.errors++ < 10) fprintf(stderr, "%s: nof_prb %u nslot %u l0 %u: %u vs %u\n", what, nprb, nslot, l0, a, b);
}

static void set_run(uint32_t m[4], uint32_t start, uint32_t len)
{
  for (uint32_t p = start; p < start + len; p++) m[p >> 5] |= 1u << (p & 31);
}

static void check(Tally& t, const uint32_t mask[2][4], uint32_t l0, uint32_t nslot, uint32_t nprb)
{
  t.cases++;
  // the allocated (symbol, PRB) pairs in mapping order
  std::vector<std::pair<uint32_t, uint32_t>> want;
  for (uint32_t l = l0; l < 2 * nslot; l++)
    for (uint32_t prb = 0; prb < nprb; prb++)
      if ((mask[l >= nslot ? 1 : 0][prb >> 5] >> (prb & 31)) & 1u) want.push_back({l, prb});
  const LsnRowGeom g = lsn_rows_geom(mask, l0, nslot, nprb);
  if (g.rows != want.size()) { fail(t, "row count", nprb, nslot, l0, g.rows, (uint32_t)want.size()); return; }
  if (g.rows0 > g.rows) { fail(t, "rows of slot 0", nprb, nslot, l0, g.rows0, g.rows); return; }
  t.rows += g.rows;
  // the PRB lists of the two slots, as the prep kernel writes them: 0xFF where nothing is written
  uint8_t list[2][128];
  memset(list, 0xFF, sizeof list);
  for (int s = 0; s < 2; s++)
    for (uint32_t prb = 0; prb < nprb; prb++)
      if ((mask[s][prb >> 5] >> (prb & 31)) & 1u) {
        const uint32_t o = lsn_rows_ordinal(mask[s], prb);
        if (o >= g.n[s] || list[s][o] != 0xFF) { fail(t, "list entry written twice or outside the list", nprb, nslot, l0, o, g.n[s]); return; }
        list[s][o] = (uint8_t)prb;
      }
  // the work items cover rows 0 .. R-1 once, with fewer than 16 rows to spare; every row resolves to its pair
  const uint32_t items = lsn_rows_items(g);
  if ((items == 0) != (g.rows == 0) || items * LSN_ROWS_PER_ITEM < g.rows || items * LSN_ROWS_PER_ITEM - g.rows >= LSN_ROWS_PER_ITEM || items > 256)
    fail(t, "item count", nprb, nslot, l0, items, g.rows);
  std::vector<uint8_t> seen(g.rows, 0);
  for (uint32_t it = 0; it < items; it++)
    for (uint32_t sub = 0; sub < LSN_ROWS_PER_ITEM; sub++) {
      const uint32_t row = it * LSN_ROWS_PER_ITEM + sub;
      if (row >= g.rows) continue;   // (the kernel's lanes of such a row leave)
      if (seen[row]++) fail(t, "row covered twice", nprb, nslot, l0, row, 0);
      uint32_t l, slot, ord;
      lsn_rows_locate(g, l0, nslot, row, &l, &slot, &ord);
      if (slot != (l >= nslot ? 1u : 0u) || slot > 1 || ord >= g.n[slot]) { fail(t, "slot / ordinal", nprb, nslot, l0, slot, ord); continue; }
      if (l != want[row].first) fail(t, "symbol of a row", nprb, nslot, l0, l, want[row].first);
      if (list[slot][ord] != want[row].second) fail(t, "PRB of a row", nprb, nslot, l0, list[slot][ord], want[row].second);
      if (row == g.rows0 && (slot != 1 || l != nslot || ord != 0)) fail(t, "first row of slot 1", nprb, nslot, l0, l, ord);
    }
  for (uint32_t row = 0; row < g.rows; row++)
    if (seen[row] != 1) fail(t, "row not covered", nprb, nslot, l0, row, seen[row]);
}

static uint32_t rng(uint64_t& s)
{
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(s >> 33);
}

int main()
{
  const uint32_t prbs[7] = {6, 15, 25, 50, 75, 100, 110};
  const uint32_t nslots[2] = {7, 6};
  Tally runs, rbg, differ, empty, divide, example;

  // the division by a slot's PRB count at every row index a job can have
  for (uint32_t n = 1; n <= 110; n++) {
    uint32_t m[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    set_run(m[0], 0, n);
    const LsnRowGeom g = lsn_rows_geom(m, 1, 7, 110);
    divide.cases++;
    for (uint32_t r = 0; r < 14 * 110; r++) {
      divide.rows++;
      if (((r * g.div_m[0]) >> LSN_ROWS_DIV_SHIFT) != r / n) fail(divide, "division", n, 7, 1, r, n);
    }
  }

  for (uint32_t nprb : prbs)
    for (uint32_t nslot : nslots)
      for (uint32_t l0 = 1; l0 <= 4; l0++) {
        // every contiguous run, the same in both slots
        for (uint32_t start = 0; start < nprb; start++)
          for (uint32_t len = 1; start + len <= nprb; len++) {
            uint32_t m[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            set_run(m[0], start, len); set_run(m[1], start, len);
            check(runs, m, l0, nslot, nprb);
          }
        // seeded RBG bitmaps with gaps (resource allocation type 0: RBGs of P PRBs, the last one short)
        const uint32_t P = nprb <= 10 ? 1 : (nprb <= 26 ? 2 : (nprb <= 63 ? 3 : 4));
        uint64_t seed = 1000003ull * nprb + 101ull * nslot + l0;
        for (int q = 0; q < 40; q++) {
          uint32_t m[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
          const uint32_t dens = 1 + rng(seed) % 7;
          for (uint32_t b = 0; b < nprb; b += P)
            if (rng(seed) % 8 < dens) { const uint32_t len = b + P <= nprb ? P : nprb - b; set_run(m[0], b, len); set_run(m[1], b, len); }
          check(rbg, m, l0, nslot, nprb);
        }
        // masks that differ between the slots: a run that hops, two unrelated bitmaps, and a slot without any PRB
        for (int q = 0; q < 40; q++) {
          uint32_t m[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
          const uint32_t len = 1 + rng(seed) % nprb, s0 = rng(seed) % (nprb - len + 1), s1 = rng(seed) % (nprb - len + 1);
          set_run(m[0], s0, len); set_run(m[1], s1, len);
          check(differ, m, l0, nslot, nprb);
          uint32_t r[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
          for (int s = 0; s < 2; s++)
            for (uint32_t p = 0; p < nprb; p++)
              if (rng(seed) & 1u) r[s][p >> 5] |= 1u << (p & 31);
          check(differ, r, l0, nslot, nprb);
          uint32_t z0[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, z1[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
          set_run(z0[1], s1, len); set_run(z1[0], s0, len);
          check(differ, z0, l0, nslot, nprb);
          check(differ, z1, l0, nslot, nprb);
        }
        uint32_t none[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        check(empty, none, l0, nslot, nprb);
        if (lsn_rows_items(lsn_rows_geom(none, l0, nslot, nprb)) != 0) fail(empty, "items of the empty allocation", nprb, nslot, l0, 1, 0);
      }

  // a job at PRBs 12-19 of a 100-PRB cell takes ceil(8 (14 - l0) / 16) work items
  for (uint32_t l0 = 1; l0 <= 4; l0++) {
    uint32_t m[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    set_run(m[0], 12, 8); set_run(m[1], 12, 8);
    const uint32_t items = lsn_rows_items(lsn_rows_geom(m, l0, 7, 100)), want = (8 * (14 - l0) + 15) / 16;
    example.cases++; example.rows += 8 * (14 - l0);
    if (items != want) fail(example, "items of PRBs 12-19", 100, 7, l0, items, want);
  }
  // the arena part of a job holds the tables and both lists
  for (uint32_t nprb : prbs)
    if (lsn_rows_sym_off(nprb) != 14 * nprb || lsn_rows_list_off(nprb) != 14 * nprb + 16 || 2 * lsn_rows_prefix_len(nprb) < 2 * lsn_rows_list_off(nprb) + 2 * nprb)
      fail(example, "arena layout", nprb, 0, 0, lsn_rows_prefix_len(nprb), lsn_rows_list_off(nprb));

  const struct { const char* name; const Tally* t; } out[6] = {{"division", &divide}, {"runs", &runs}, {"rbg", &rbg}, {"differ", &differ}, {"empty", &empty}, {"example", &example}};
  long errors = 0;
  for (const auto& o : out) {
    printf("%s: %ld cases %ld rows %ld errors\n", o.name, o.t->cases, o.t->rows, o.t->errors);
    errors += o.t->errors;
  }
  return errors ? 1 : 0;
}

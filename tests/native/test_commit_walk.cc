// Stand-alone run of the product's commit walk (csrc/host/lsn_commit.h) with a scripted decoder, meant to be built with -fsanitize=address,undefined: random DCIs
// through FalconSearch::finishSubframe, the commit view and the walk, with the tracking database off, on and in both-tables mode, and with HARQ on; the database
// is aged now and then.  Checks what must hold whatever the DCIs say (records only of passed blocks, lengths inside the payload store); prints OK.
#include "commit_script_host.h"
#include <cstdio>
#include <cstdlib>

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((rng_state >> 33) % n); }
static uint64_t mix(uint64_t a, uint64_t b) { uint64_t x = (a ^ b) * 0xBF58476D1CE4E5B9ull; return x ^ (x >> 29); }
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s (line %d)\n", #x, __LINE__); exit(1); } } while (0)

// a MAC PDU whose one CCCH SDU (LCID 0, rest padding) is NOT a connection setup, a random-access response, or bytes: a pure function of (tti, RNTI, block, size)
static int script(void* user, const uint32_t* call, float, uint8_t* pl0, uint8_t* pl1, int32_t* crc)
{
  uint64_t& ncalls = *(uint64_t*)user;
  ncalls++;
  uint8_t* pl[2] = {pl0, pl1};
  for (int tb = 0; tb < 2; tb++) {
    const uint32_t en = call[6 + 5 * tb], tbs = call[8 + 5 * tb];
    crc[tb] = 0;
    if (!(en && tbs > 0)) continue;
    uint64_t h = mix(mix(mix(call[0], call[1]), (uint64_t)tb), tbs);
    crc[tb] = (h % 100) < 55;
    const uint32_t n = tbs / 8;
    CHECK(n <= CommitScriptHost::TB_STRIDE);
    for (uint32_t i = 0; i < n; i++) { h = mix(h, i); pl[tb][i] = (uint8_t)h; }
    if (call[1] >= 1 && call[1] <= 10 && n >= 7) { pl[tb][0] = 0x40 | (uint8_t)(h & 0x3F); pl[tb][5] = (uint8_t)(1 + (h >> 8) % 200); }   // E = 0, T = 1, RAPID; a temporary C-RNTI above the RA-RNTIs
    else if ((h >> 20) % 3 == 0 && n >= 2) { pl[tb][0] = 0x20; pl[tb][1] = 0x1F; }   // E = 1, LCID 0 without length field is not legal: the parser must cope
  }
  return 0;
}

static uint64_t run(uint32_t nof_prb, uint32_t nof_ports, uint32_t cp, int mode, int harq, uint32_t nof_rx, uint32_t nsf, uint64_t& ncalls)
{
  hcommit h;
  commit_script_init(h, nof_prb, nof_ports, 3, cp, mode, harq, nof_rx);
  h.script = script; h.script_user = &ncalls;
  uint16_t ues[12];
  for (auto& u : ues) u = (uint16_t)(0x0100 + rnd(0xFE00));
  std::vector<std::vector<uint32_t>> old_meta(8);
  std::vector<std::vector<uint8_t>> old_bits(8);
  uint64_t nrec = 0;
  uint32_t tti = rnd(10240);
  for (uint32_t k = 1; k <= nsf; k++) {
    tti = (tti + 1) % 10240;
    h.now = k * 40;   // (40 subframes per step: the 5 s interval of the tracking database passes inside the run)
    if (k % 61 == 0) h.mcs.update_database_dl(h.now);
    if (harq && k % 97 == 0) h.harq.update_database(h.now);
    std::vector<uint32_t> meta;
    std::vector<uint8_t> bits;
    const uint32_t n = rnd(8);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t u = rnd(100);
      uint32_t rnti, fmt;
      if (u < 15) { const uint16_t common[4] = {SIRNTI, PRNTI, (uint16_t)(1 + rnd(10)), 0}; rnti = common[rnd(4)]; fmt = rnd(2) ? FORMAT1A : FORMAT1C; }
      else if (u < 20) { rnti = rnd(65536); fmt = rnd(NOF_FORMATS); }
      else { rnti = ues[rnd(12)]; fmt = rnd(NOF_FORMATS); }
      const uint32_t nb = dci_format_sizeof(h.cell, (DciFormat)fmt);
      CHECK(nb > 0 && nb <= 64);
      const uint32_t L = rnd(4);
      const uint32_t m[6] = {rnti, fmt, L, (rnd(80) >> L) << L, rnd(40), nb};
      meta.insert(meta.end(), m, m + 6);
      const size_t at = bits.size();
      bits.resize(at + 128, 0);
      for (uint32_t b = 0; b < nb; b++) bits[at + b] = (uint8_t)rnd(2);
      if (fmt == FORMAT0) bits[at] = 0;
      if (fmt == FORMAT1A) bits[at] = 1;
    }
    if (harq && rnd(10) < 6) {  // retransmissions: the grants of 8 subframes ago again, bit for bit
      const auto& om = old_meta[k % 8]; const auto& ob = old_bits[k % 8];
      for (size_t i = 0; i < om.size() / 6 && meta.size() / 6 < 12; i++)
        if (om[6 * i + 1] != FORMAT0 && rnd(10) < 7) { meta.insert(meta.end(), om.begin() + 6 * i, om.begin() + 6 * i + 6); bits.insert(bits.end(), ob.begin() + 128 * i, ob.begin() + 128 * i + 128); }
    }
    old_meta[k % 8] = meta; old_bits[k % 8] = bits;
    meta.resize(meta.size() + 6); bits.resize(bits.size() + 128);   // (never empty: data() of an empty vector may be null)
    commit_script_subframe(h, tti / 10, tti % 10, 1 + rnd(3), (uint32_t)(old_meta[k % 8].size() / 6), meta.data(), bits.data());
    for (const hcommit::Rec& r : h.recs) {
      CHECK(r.kind >= 1 && r.kind <= 4 && r.tti == tti && r.len > 0 && (size_t)r.off + r.len <= h.payload.size());
      nrec++;
    }
    for (const JobRes& jr : h.jres)
      for (int tb = 0; tb < 2; tb++) CHECK(!jr.crc[tb] || (jr.enabled[tb] && jr.len[tb] >= 0));
  }
  return nrec;
}

int main()
{
  uint64_t ncalls = 0, nrec = 0;
  nrec += run(100, 2, 0, 0, 0, 2, 300, ncalls);
  nrec += run(50, 2, 0, 1, 0, 1, 300, ncalls);
  nrec += run(25, 1, 0, 1, 0, 2, 300, ncalls);
  nrec += run(75, 2, 1, 2, 0, 2, 300, ncalls);
  nrec += run(15, 4, 0, 1, 0, 2, 300, ncalls);
  nrec += run(100, 2, 0, 0, 1, 2, 400, ncalls);
  nrec += run(50, 2, 0, 1, 1, 2, 400, ncalls);
  if (ncalls < 2000 || nrec < 1000) { fprintf(stderr, "FAILED: %llu decode calls, %llu records - the walk hardly ran\n", (unsigned long long)ncalls, (unsigned long long)nrec); return 1; }
  printf("OK %llu decode calls, %llu records\n", (unsigned long long)ncalls, (unsigned long long)nrec);
  return 0;
}

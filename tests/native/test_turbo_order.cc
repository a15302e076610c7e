// Stand-alone check of turbo_packed_order / turbo_place (lsn_lte.cc), meant to be built with -fsanitize=address,undefined: the counting sort indexes a table by
// (phase, class, K), and the placement writes one descriptor per block.  Compared with a plain stable sort of the same key; prints OK.
#include "../../ltesniffer_amd/csrc/host/lsn_lte.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
using namespace lsn;

static std::vector<uint32_t> legal_k()
{
  std::vector<uint32_t> v;
  for (uint32_t k = 40; k <= 6144; k += k < 512 ? 8 : k < 1024 ? 16 : k < 2048 ? 32 : 64) v.push_back(k);
  return v;
}
static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((rng_state >> 33) % n); }
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s (line %d, set of %zu)\n", #x, __LINE__, cbs.size()); exit(1); } } while (0)

static void check(const std::vector<LsnCbDev>& cbs)
{
  const uint32_t n = (uint32_t)cbs.size();
  std::vector<uint32_t> want(n);
  for (uint32_t i = 0; i < n; i++) want[i] = i;
  auto phase = [&](uint32_t i) { return cbs[i].dep != LSN_CB_NODEP ? 1u : 0u; };
  auto pair = [&](uint32_t i) { return cbs[i].K <= LSN_TURBO_PAIR_KMAX && turbo_nwin((int)cbs[i].K) <= 64; };
  std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) {
    if (phase(x) != phase(y)) return phase(x) < phase(y);
    if (pair(x) != pair(y)) return !pair(x);
    return cbs[x].K > cbs[y].K;
  });
  uint32_t nsolo[2] = {0, 0}, npair[2] = {0, 0}, kmax_solo = 0, kmax_pair = 0, emax = 0;
  size_t words = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (pair(i)) { npair[phase(i)]++; kmax_pair = std::max(kmax_pair, cbs[i].K); } else { nsolo[phase(i)]++; kmax_solo = std::max(kmax_solo, cbs[i].K); }
    emax = std::max(emax, cbs[i].E);
    words += LSN_SPP_WORDS(cbs[i].K);
  }
  const TurboPackedOrder o = turbo_packed_order(cbs);
  CHECK(o.order == want);
  CHECK(o.nsolo[0] == nsolo[0] && o.nsolo[1] == nsolo[1] && o.npair[0] == npair[0] && o.npair[1] == npair[1]);
  CHECK(o.kmax_solo == kmax_solo && o.kmax_pair == kmax_pair);
  std::vector<LsnCbDev> dst(n);   // exactly n descriptors: a write past the end is the sanitizer's to find
  const uint32_t base = 4 * rnd(64);
  const TurboPlacement p = turbo_place(cbs, o.order, base, dst.data());
  CHECK(p.spp_n == words && p.emax == emax && p.spp_of.size() == n);
  uint32_t at = base;
  for (uint32_t i = 0; i < n; i++) {
    CHECK(dst[i].spp_off == at && (at & 3u) == 0 && dst[i].K == cbs[want[i]].K && dst[i].res_idx == want[i] && p.spp_of[want[i]] == at);
    at += LSN_SPP_WORDS(dst[i].K);
  }
}

int main()
{
  const std::vector<uint32_t> ks = legal_k();
  if (ks.size() != 188) { fprintf(stderr, "FAILED: %zu block sizes\n", ks.size()); return 1; }
  auto block = [](uint32_t K, uint32_t dep, uint32_t idx) { LsnCbDev c{}; c.K = K; c.dep = dep; c.E = 1 + rnd(30000); c.res_idx = idx; return c; };
  std::vector<LsnCbDev> cbs;
  check(cbs);                                                    // empty
  for (uint32_t k : ks) { cbs.assign(1, block(k, LSN_CB_NODEP, 0)); check(cbs); }   // every size alone
  cbs.clear();
  for (uint32_t i = 0; i < ks.size(); i++) cbs.push_back(block(ks[i], i & 1 ? 0u : LSN_CB_NODEP, i));   // every size, both phases
  check(cbs);
  for (int trial = 0; trial < 300; trial++) {
    const uint32_t n = rnd(401), mode = (uint32_t)trial % 4;      // mode 0: all independent, 1: all but one dependent, 2 / 3: mixed
    cbs.clear();
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t K = trial % 3 == 0 ? ks[rnd(8) * 23] : ks[rnd(188)];   // (few sizes: many equal K)
      const bool dependant = mode == 0 ? false : mode == 1 ? i != 0 : i != 0 && rnd(3) != 0;
      cbs.push_back(block(K, dependant ? rnd(i) : LSN_CB_NODEP, i));
    }
    check(cbs);
  }
  printf("OK\n");
  return 0;
}

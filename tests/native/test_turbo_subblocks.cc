// CPU checks of the turbo decoder's sub-block schedule (ltesniffer_amd/csrc/kernels/lsn_turbo_core.h: the short sub-block of a window comes FIRST):
//   geometry - for every legal block size the sub-blocks tile the window, the last one is full, and a pass runs W - 16 forward-sweep steps
//              (counted in the decoder's own text, per lane, and from its geometry helper);
//   table    - for every block size, window and step the half-word the decoder reads from the interleaver address table is the transposed address of
//              pi(w W + t), pi from the QPP parameters by brute force; every half-word no step reads is an address inside the block;
//   second   - the decoder text as the SECOND block of a paired workgroup gets it (TurboLds::bias / cw / ch non-zero) against the oracle's decoder,
//              range checks on, with the first block's half of every array watched for stray writes.
// Built by tests/test_turbo_subblocks.py with the clang++ of tests/native/Makefile; links the oracle.  The encoder, the termination metrics and the random
// numbers are those of test_turbo_core.cc (its main is not used).
static long g_fwd_sweep_steps = 0;
#define LSN_FWD_SWEEP_COUNT(n) (g_fwd_sweep_steps += (n))
#define main test_turbo_core_main
#include "test_turbo_core.cc"
#undef main
#include <set>

static std::vector<int> legal_sizes()
{
  std::vector<int> Ks;
  for (int K = 40; K <= 512; K += 8) Ks.push_back(K);
  for (int K = 528; K <= 1024; K += 16) Ks.push_back(K);
  for (int K = 1056; K <= 2048; K += 32) Ks.push_back(K);
  for (int K = 2112; K <= 6144; K += 64) Ks.push_back(K);
  return Ks;
}

static int check_geometry()
{
  int bad = 0, shortened = 0;
  for (int K : legal_sizes()) {
    const int P = lsn_turbo_nwin(K), W = K / P, nsb = lsn_turbo_nsb(W);
    int at = 0, ok = nsb >= 2;
    for (int sb = 0; sb < nsb; sb++) {
      const LsnSubBlock s = lsn_turbo_sb(W, sb);
      ok = ok && s.start == at && s.len >= 1 && s.len <= TB_S && (sb == 0 || s.len == TB_S);
      for (int t = s.start; t < s.start + s.len; t++) ok = ok && lsn_turbo_sb_of(W, t) == sb;
      at += s.len;
    }
    ok = ok && at == W && lsn_turbo_sb(W, nsb - 1).len == TB_S && lsn_turbo_sb(W, nsb - 1).start == W - TB_S;
    ok = ok && lsn_turbo_fwd_steps(W) == W - TB_S;
    shortened += (W % TB_S) != 0;
    if (!ok) { std::fprintf(stderr, "GEOMETRY K=%d W=%d: sub-blocks do not tile the window with a full last one / %d forward-sweep steps\n", K, W, lsn_turbo_fwd_steps(W)); bad++; }
  }
  std::printf("geometry: %zu sizes, %d with a short sub-block, %d bad\n", legal_sizes().size(), shortened, bad);
  return bad;
}

static int check_table()
{
  int bad = 0;
  long halves = 0, unused = 0;
  for (int K : legal_sizes()) {
    const int P = lsn_turbo_nwin(K), W = K / P, nw = (W + 1) / 2;
    int f1, f2;
    if (o_qpp_find(K, &f1, &f2) < 0) { std::fprintf(stderr, "TABLE K=%d: no QPP parameters\n", K); bad++; continue; }
    if (lsn_turbo_il_words(K) != nw * P) { std::fprintf(stderr, "TABLE K=%d: %d words\n", K, lsn_turbo_il_words(K)); bad++; continue; }
    std::vector<uint32_t> il(nw * P + 16, 0xFFFFFFFFu);
    lsn_turbo_il_fill(il.data(), K, f1, f2);
    for (int i = 0; i < 16; i++) if (il[nw * P + i] != 0xFFFFFFFFu) { std::fprintf(stderr, "TABLE K=%d: written past its %d words\n", K, nw * P); bad++; break; }
    std::set<long> read;
    int kbad = 0;
    for (int w = 0; w < P; w++)
      for (int t = 0; t < W; t++) {
        // what lsn_map_pass_lane reads for step t: word (first word of the sub-block + u / 2) of column w, half u & 1, u = step inside the sub-block
        const LsnSubBlock s = lsn_turbo_sb(W, lsn_turbo_sb_of(W, t));
        const int u = t - s.start, word = (s.word + (u >> 1)) * P + w;
        if (word < 0 || word >= nw * P) { kbad++; continue; }
        const int got = (int)((il[word] >> (16 * (u & 1))) & 0xFFFFu);
        const unsigned long long x = (unsigned long long)w * W + t;
        const int pi = (int)(((unsigned long long)f1 * x + (unsigned long long)f2 * x * x) % (unsigned long long)K);
        if (got != (pi % W) * P + pi / W) kbad++;
        if (!read.insert(2l * word + (u & 1)).second) kbad++;   // two steps in one half-word
        halves++;
      }
    for (long h = 0; h < 2l * nw * P; h++)
      if (!read.count(h)) {
        unused++;
        if ((int)((il[h >> 1] >> (16 * (h & 1))) & 0xFFFFu) >= K) kbad++;
      }
    if (kbad) { std::fprintf(stderr, "TABLE K=%d W=%d P=%d: %d wrong half-words\n", K, W, P, kbad); bad++; }
  }
  std::printf("table: %ld half-words read, %ld unused, %d bad sizes\n", halves, unused, bad);
  return bad;
}

// the kernel's text for the second block of a paired workgroup (stage_c.hip: k_turbo, paired), lane by lane; the first block's halves hold a pattern
static int decode_second_half(const int16_t* d3, int K, int max_iter, uint32_t poly, uint8_t* bits, int* ok_out, int* stray)
{
  constexpr int NT = 64;
  const int D = K + 4, P = lsn_turbo_nwin(K), W = K / P;
  int f1, f2;
  o_qpp_find(K, &f1, &f2);
  const uint32_t magicW = ((1u << 20) + (uint32_t)W - 1u) / (uint32_t)W;
  std::vector<uint32_t> il(lsn_turbo_il_words(K));
  lsn_turbo_il_fill(il.data(), K, f1, f2);
  const int kmax = ((K < 512 ? 512 : K) + 7) & ~7, kk = kmax + 8;
  const uint32_t PAT32 = 0xA5C3F00Fu;
  const int16_t PAT16 = (int16_t)0x5AA5;
  std::vector<uint32_t> spp(2 * kk + 256, PAT32);
  std::vector<int16_t> ext(2 * kk + 256, PAT16);
  std::vector<uint8_t> ckpt(2 * TB_CKPT_BYTES + 64, 0xC7);
  TurboLds m;
  m.spp = spp.data(); m.ext = ext.data(); m.ckpt = ckpt.data();
  m.bias = kk; m.cw = (int)(TB_CKPT_BYTES / 4); m.ch = 2 * m.cw;
  const int16_t *d0 = d3, *d1 = d3 + D, *d2 = d3 + 2 * D;
  for (int t = 0; t < K; t++) {
    const int x = (t % P) * W + t / P;
    spp[m.bias + t] = ((uint32_t)d0[x] & 0x3FFu) | (((uint32_t)d1[x] & 0x3FFu) << 10) | (((uint32_t)d2[x] & 0x3FFu) << 20);
    ext[m.bias + t] = 0;
  }
  int tail[12];
  for (int s = 0; s < 3; s++) for (int j = 0; j < 4; j++) tail[s * 4 + j] = (s == 0 ? d0 : s == 1 ? d1 : d2)[K + j];
  int bt1i[8], bt2i[8];
  {
    const int *s4 = tail, *q1 = tail + 4, *q2 = tail + 8;
    int ts1[3] = {s4[0], q2[0], q1[1]}, tp1[3] = {q1[0], s4[1], q2[1]};
    int ts2[3] = {s4[2], q2[2], q1[3]}, tp2[3] = {q1[2], s4[3], q2[3]};
    tail_beta(ts1, tp1, bt1i);
    tail_beta(ts2, tp2, bt2i);
  }
  s2 bt1[4], bt2[4];
  lsn_pack_c(bt1i, bt1); lsn_pack_c(bt2i, bt2);
  std::vector<s2> na1(4 * NT, s2{0, 0}), nb1(4 * NT, s2{0, 0}), na2(4 * NT, s2{0, 0}), nb2(4 * NT, s2{0, 0}), ae(4 * NT), bo(4 * NT);
  auto pass = [&](bool second, std::vector<s2>& na, std::vector<s2>& nb, const s2* bt) {
    for (int lane = 0; lane < NT; lane++) {
      for (int k = 0; k < 4; k++) ae[4 * lane + k] = bo[4 * lane + k] = s2{0, 0};
      if (lane >= P) continue;
      const long before = g_fwd_sweep_steps;
      if (second) lsn_map_pass_lane<true>(m, il.data(), NT, lane, K, P, W, &na[4 * lane], &nb[4 * lane], bt, &ae[4 * lane], &bo[4 * lane]);
      else lsn_map_pass_lane<false>(m, il.data(), NT, lane, K, P, W, &na[4 * lane], &nb[4 * lane], bt, &ae[4 * lane], &bo[4 * lane]);
      if (g_fwd_sweep_steps - before != W - TB_S) { std::fprintf(stderr, "K=%d lane %d: %ld forward-sweep steps in a pass, W = %d\n", K, lane, g_fwd_sweep_steps - before, W); (*stray)++; }
    }
    for (int lane = 0; lane < NT; lane++) { lsn_ckpt_store(m.ckpt, NT, 0, lane, &ae[4 * lane], m.cw, m.ch); lsn_ckpt_store(m.ckpt, NT, 1, lane, &bo[4 * lane], m.cw, m.ch); }
    for (int lane = 0; lane < NT; lane++) {
      const int lm = lane > 0 ? lane - 1 : 0, lq = lane + 1 < NT ? lane + 1 : lane;
      lsn_ckpt_load(m.ckpt, NT, 0, lm, &na[4 * lane], m.cw, m.ch);
      lsn_ckpt_load(m.ckpt, NT, 1, lq, &nb[4 * lane], m.cw, m.ch);
    }
  };
  int it = 0, ok = 0;
  while (it < max_iter && !ok) {
    pass(false, na1, nb1, bt1);
    pass(true, na2, nb2, bt2);
    it++;
    for (int x = 0; x < K; x++) bits[x] = (uint8_t)(ext[m.bias + tr_idx(x, W, P, magicW)] & 1);
    ok = o_crc_bits(poly, 24, bits, K) == 0;
  }
  // nothing of the first block's half may have been written
  for (int i = 0; i < kk; i++) *stray += (spp[i] != PAT32) + (ext[i] != PAT16);
  for (size_t i = 0; i < TB_CKPT_BYTES; i++) *stray += ckpt[i] != 0xC7;
  *ok_out = ok;
  return it;
}

static int check_second_half()
{
  const int sizes[4] = {256, 264, 400, 376};   // W mod 16 = 0, 1, 8, 15 (W = 32, 33, 40, 47), all K <= 2752: blocks the host pairs
  int bad = 0, n = 0, several = 0;
  long iters = 0;
  for (int K : sizes) {
    const int D = K + 4, W = K / lsn_turbo_nwin(K);
    int f1, f2;
    if (o_qpp_find(K, &f1, &f2) < 0) { bad++; continue; }
    for (int rep = 0; rep < 6; rep++)
      for (int kind = 0; kind < 2; kind++) {   // a marginal code word; saturated noise
        std::vector<int16_t> d3(3 * D);
        std::vector<uint8_t> c(K), ba(K), bb(K);
        const uint32_t poly = (rep & 1) ? 0x1800063u : 0x1864CFBu;
        if (kind == 0) {
          for (int i = 0; i < K - 24; i++) c[i] = (uint8_t)(rnd() & 1);
          const uint32_t r = o_crc_bits(poly, 24, c.data(), K - 24);   // (appends the 24 zeros itself)
          for (int i = 0; i < 24; i++) c[K - 24 + i] = (uint8_t)((r >> (23 - i)) & 1);
          encode(c.data(), K, f1, f2, d3.data(), 64.0, 58.0 + (rnd() % 24));   // around the threshold of these short blocks: some decode late, some never
        } else {
          for (auto& v : d3) v = (int16_t)((rnd() & 1) ? 511 : -511);
        }
        int oka = 0, okb = 0, stray = 0;
        const int ia = o_turbo_decode_cb(d3.data(), K, 12, poly, ba.data(), &oka);
        const int ib = decode_second_half(d3.data(), K, 12, poly, bb.data(), &okb, &stray);
        iters += ib; n++;
        several += kind == 0 && ib >= 3 && okb;
        if (ia != ib || oka != okb || memcmp(ba.data(), bb.data(), K) != 0 || stray) {
          std::fprintf(stderr, "SECOND HALF K=%d (W mod 16 = %d) kind=%d: oracle it=%d ok=%d, kernel text it=%d ok=%d, %d stray writes / step-count errors\n", K, W % TB_S, kind, ia, oka, ib, okb, stray);
          bad++;
        }
      }
  }
  std::printf("second half: %d cases, %ld iterations, %d code words decoded in three or more, %d bad\n", n, iters, several, bad);
  return bad;
}

int main()
{
  const int bad = check_geometry() + check_table() + check_second_half();
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

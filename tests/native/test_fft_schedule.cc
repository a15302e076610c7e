// The symbol transform's schedule (ltesniffer_amd/csrc/kernels/lsn_fft_map.h) replayed on the CPU: a loop over the 256 threads, pass by pass, a plain array
// for LDS, every index taken from the header the kernels index with.  A program of its own (tests/test_fft_schedule.py builds and runs it; link with the
// oracle library, compile with -ffp-contract=off).  Lines "name: <cases> cases <words> words <errors> errors"; "bank" lines carry the LDS model's cycles.
//   exact   N = 128 .. 2048 and 1536 against o_fft, word for word
//   three   the three-way formula restated on o_fft(M): equals o_fft(1536) at M = 512; the schedule equals it at 384 and 768
//   bank    ds_read_b64: 2 groups of 32 lanes, bank = dword mod 64; ds_write_b64: 4 groups of 16 lanes, bank = dword mod 32 (distinct addresses on one bank
//           serialise, equal addresses broadcast): reads conflict-free, writes at most 2-way; the same count for the map before (base + j h, brev(n))
//   cover   every kept carrier is written once by the last pass; no LDS slot beyond the declared size
#include "../../ltesniffer_amd/csrc/kernels/lsn_fft_map.h"
#include "../../oracle/lsn_oracle.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

typedef ocf_t cf;
static inline cf cmul(cf a, cf b) { cf c; c.r = a.r * b.r - a.i * b.i; c.i = a.r * b.i + a.i * b.r; return c; }

struct Size { int N, nb, lgM; };
static const Size SIZES[8] = {{128, 1, 7}, {256, 1, 8}, {512, 1, 9}, {1024, 1, 10}, {2048, 1, 11}, {384, 3, 7}, {768, 3, 8}, {1536, 3, 9}};

// one LDS access of one wave-instruction: slot per thread, -1 = lane off
struct Access { bool write; std::vector<int> slot; };
struct Trace { std::vector<Access> acc; int max_slot = -1; };

static void butterflies(cf* e, int R, int s, int low, int lgM, const cf* W)
{
  for (int q = 0; q < R; q++)
    for (int j = 0; j < (1 << R); j++) {
      if (j & (1 << q)) continue;
      const int m = j & ((1 << q) - 1);
      const cf v = cmul(e[j + (1 << q)], W[lsn_fft_twiddle(low + (m << s), s + q, lgM)]);
      const cf u = e[j];
      e[j].r = u.r + v.r; e[j].i = u.i + v.i;
      e[j + (1 << q)].r = u.r - v.r; e[j + (1 << q)].i = u.i - v.i;
    }
}

// The schedule.  x: N time samples; W: M / 2 twiddles; T: N twiddles of the combine (nb = 3).  bins (N values, natural order) receives what the last pass /
// the combine holds for every bin; written[bin] counts the writes.  tr (optional) records every LDS access.  Returns the LDS image's slot count in use.
static void run_schedule(const Size& z, const cf* x, const cf* W, const cf* T, cf* bins, int* written, Trace* tr, long* errors)
{
  const int N = z.N, nb = z.nb, lgM = z.lgM, M = 1 << lgM, LDS = lsn_fft_lds_slots(N);
  std::vector<cf> lds((size_t)LDS);
  std::vector<char> filled((size_t)LDS, 0);
  auto slot_ok = [&](int sl) { if (sl < 0 || sl >= LDS) { ++*errors; return false; } if (tr && sl > tr->max_slot) tr->max_slot = sl; return true; };
  auto record = [&](bool write, const std::vector<int>& v) { if (tr) tr->acc.push_back(Access{write, v}); };
  // pass 0
  {
    std::vector<std::vector<int>> w(8, std::vector<int>(LSN_FFT_THREADS, -1));
    for (int t = 0; t < LSN_FFT_THREADS && t < N / 8; t++) {
      cf ld[8], e[8];
      for (int jj = 0; jj < 8; jj++) ld[jj] = x[lsn_fft_first_sample(t, jj, N)];
      for (int j = 0; j < 8; j++) e[j] = ld[lsn_fft_brev3(j)];
      butterflies(e, 3, 0, 0, lgM, W);
      int r, g;
      lsn_fft_first_group(t, nb, lgM, &r, &g);
      const int at = lsn_fft_store(r, 8 * g, lgM);
      for (int j = 0; j < 8; j++) {
        const int sl = at ^ lsn_fft_slot(j);
        if (sl != lsn_fft_store(r, 8 * g + j, lgM)) ++*errors;  // the linearity the kernel relies on
        if (!slot_ok(sl)) continue;
        if (filled[sl]) ++*errors;
        filled[sl] = 1; lds[sl] = e[j]; w[j][t] = sl;
      }
    }
    for (int j = 0; j < 8; j++) record(true, w[j]);
    for (int sl = 0; sl < nb * M; sl++) if (!filled[sl]) ++*errors;  // the map is onto
  }
  for (int s = 3; s < lgM;) {
    const int R = lsn_fft_radix(lgM, s), G = 1 << R, ng = lsn_fft_groups(nb, lgM, R);
    const bool last = s + R == lgM, to_bins = last && nb == 1;
    std::vector<cf> next = lds;  // a pass reads what the barrier before it left: writes go to a copy
    for (int u = 0; u * LSN_FFT_THREADS < ng; u++) {
      std::vector<std::vector<int>> a(G, std::vector<int>(LSN_FFT_THREADS, -1));
      for (int t = 0; t < LSN_FFT_THREADS; t++) {
        const int gg = t + LSN_FFT_THREADS * u;
        if (gg >= ng) continue;
        const int r = gg >> (lgM - R), g = gg & ((1 << (lgM - R)) - 1), base = lsn_fft_base(g, s, R), at = lsn_fft_store(r, base, lgM);
        cf e[8];
        for (int j = 0; j < G; j++) {
          const int sl = at ^ lsn_fft_slot(j << s);
          if (sl != lsn_fft_store(r, base + (j << s), lgM)) ++*errors;
          a[j][t] = sl;
          e[j] = slot_ok(sl) ? lds[sl] : cf{0, 0};
        }
        butterflies(e, R, s, base & ((1 << s) - 1), lgM, W);
        for (int j = 0; j < G; j++) {
          if (to_bins) {
            const int bin = g + (j << s);
            int ot, ou, oj;
            lsn_fft_last_owner(bin, lgM, R, &ot, &ou, &oj);
            if (ot != t || ou != u || oj != j) ++*errors;
            bins[bin] = e[j]; written[bin]++;
          } else if (slot_ok(a[j][t])) next[a[j][t]] = e[j];
        }
      }
      for (int j = 0; j < G; j++) record(false, a[j]);
      if (!to_bins) for (int j = 0; j < G; j++) record(true, a[j]);
    }
    lds = next;
    s += R;
  }
  if (nb == 3) {  // the combine over every bin (the kernel forms the kept ones)
    for (int bin = 0; bin < N; bin++) {
      const int kq = bin & (M - 1);
      int b2 = 2 * bin;
      b2 = b2 >= N ? b2 - N : b2;
      const cf f0 = lds[lsn_fft_store(0, kq, lgM)];
      const cf t1 = cmul(lds[lsn_fft_store(1, kq, lgM)], T[bin]), t2 = cmul(lds[lsn_fft_store(2, kq, lgM)], T[b2]);
      const float sr = f0.r + t1.r, si = f0.i + t1.i;
      bins[bin].r = sr + t2.r; bins[bin].i = si + t2.i;
      written[bin]++;
    }
  }
}

// the three-way formula of lsn_dsp.h restated on the oracle's M-point transform
static void three_way(int M, const cf* W, const cf* T, const cf* x, cf* X)
{
  const int N = 3 * M;
  std::vector<cf> sub[3];
  for (int r = 0; r < 3; r++) {
    sub[r].resize((size_t)M);
    for (int m = 0; m < M; m++) sub[r][m] = x[3 * m + r];
    o_fft(M, W, sub[r].data());
  }
  for (int k = 0; k < N; k++) {
    const int kq = k % M;
    const cf t1 = cmul(sub[1][kq], T[k]), t2 = cmul(sub[2][kq], T[(2 * k) % N]);
    const float sr = sub[0][kq].r + t1.r, si = sub[0][kq].i + t1.i;
    X[k].r = sr + t2.r; X[k].i = si + t2.i;
  }
}

static uint32_t rng_state = 0x1234567u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return ((int32_t)rng_state) * (1.0f / 2147483648.0f); }

// the input rows of the issue: random, zeros, negative zeros, impulses at 0, 1, N / 2, N - 1, a row with denormals
static std::vector<std::vector<cf>> inputs(int N)
{
  std::vector<std::vector<cf>> v;
  std::vector<cf> x((size_t)N);
  for (auto& e : x) { e.r = rnd(); e.i = rnd(); }
  v.push_back(x);
  for (auto& e : x) { e.r = 0.0f; e.i = 0.0f; }
  v.push_back(x);
  for (auto& e : x) { e.r = -0.0f; e.i = -0.0f; }
  v.push_back(x);
  const int at[4] = {0, 1, N / 2, N - 1};
  for (int p = 0; p < 4; p++) {
    for (auto& e : x) { e.r = 0.0f; e.i = 0.0f; }
    x[at[p]].r = 1.0f; x[at[p]].i = -0.5f;
    v.push_back(x);
  }
  for (int n = 0; n < N; n++) { x[n].r = (n % 3 == 0) ? 1e-41f * (float)(n + 1) : rnd() * 1e-38f; x[n].i = (n % 5 == 0) ? -3e-42f : rnd() * 1e-37f; }
  v.push_back(x);
  return v;
}

static void tables(const Size& z, std::vector<cf>& W, std::vector<cf>& T)
{
  const int M = 1 << z.lgM;
  W.resize((size_t)M / 2);
  o_fft_twiddles(M, W.data());
  T.clear();
  if (z.nb == 3)
    for (int k = 0; k < z.N; k++) {  // as o_fft_twiddles builds the circle of 1536
      const double a = 2.0 * M_PI * (double)k / (double)z.N;
      T.push_back(cf{(float)cos(a), (float)(-sin(a))});
    }
}

// cycles the LDS array spends on one wave-instruction's accesses and the worst multiplicity in a lane group
static void bank_cost(const Access& a, long* cycles, long* extra, int* worst)
{
  const int gs = a.write ? 16 : 32;  // 16 lanes x 2 dwords on 32 banks; 32 lanes x 2 dwords on 64 banks: the bank pair of a cf32 slot is slot mod gs
  for (int l0 = 0; l0 < LSN_FFT_THREADS; l0 += gs) {
    int nd[32] = {0}, seen[32][32];
    bool any = false;
    for (int l = l0; l < l0 + gs; l++) {
      const int sl = a.slot[l];
      if (sl < 0) continue;
      any = true;
      const int b = sl % gs;
      bool dup = false;
      for (int k = 0; k < nd[b]; k++) dup |= seen[b][k] == sl;
      if (!dup) seen[b][nd[b]++] = sl;
    }
    if (!any) continue;
    int m = 1;
    for (int b = 0; b < gs; b++) m = nd[b] > m ? nd[b] : m;
    *cycles += m; *extra += m - 1;
    if (m > *worst) *worst = m;
  }
}

// the accesses of the schedule before: bit-reversed scatter, every pass in place at base + j h with g = tid (8 >> R) + u, gather of the carriers
static Trace old_trace(const Size& z, int nre, int dc)
{
  Trace tr;
  const int N = z.N, nb = z.nb, lgM = z.lgM, M = 1 << lgM;
  auto brev = [&](int n) { int b = 0; for (int k = 0; k < lgM; k++) b |= ((n >> k) & 1) << (lgM - 1 - k); return b; };
  for (int n0 = 0; n0 < N; n0 += 256) {
    std::vector<int> v(256, -1);
    for (int t = 0; t < 256 && n0 + t < N; t++) { const int n = n0 + t; v[t] = nb == 3 ? (n % 3) * M + brev(n / 3) : brev(n); }
    tr.acc.push_back(Access{true, v});
  }
  for (int s = 0; s < lgM;) {
    const int R = lgM - s >= 3 ? 3 : lgM - s, h = 1 << s;
    for (int r = 0; r < nb; r++)
      for (int u = 0; u < (8 >> R); u++) {
        std::vector<std::vector<int>> a(1 << R, std::vector<int>(256, -1));
        bool any = false;
        for (int t = 0; t < 256; t++) {
          const int g = t * (8 >> R) + u;
          if (g >= (M >> R)) continue;
          any = true;
          for (int j = 0; j < (1 << R); j++) a[j][t] = r * M + (((g >> s) << (s + R)) | (g & (h - 1))) + j * h;
        }
        if (!any) continue;
        for (auto& v : a) tr.acc.push_back(Access{false, v});
        for (auto& v : a) tr.acc.push_back(Access{true, v});
      }
    s += R;
  }
  for (int k0 = 0; k0 < nre; k0 += 256)
    for (int r = 0; r < nb; r++) {
      std::vector<int> v(256, -1);
      for (int t = 0; t < 256 && k0 + t < nre; t++) { const int bin = lsn_fft_carrier_bin(k0 + t, N, nre, dc); v[t] = nb == 3 ? r * M + (bin & (M - 1)) : bin; }
      tr.acc.push_back(Access{false, v});
      if (nb == 1) break;
    }
  return tr;
}

static int nre_of(int N) { return N == 128 ? 72 : N == 256 ? 180 : N == 512 || N == 384 ? 300 : N == 1024 || N == 768 ? 600 : N == 1536 ? 900 : 1200; }

int main()
{
  long total_errors = 0;
  // ---- exact: against o_fft
  {
    long cases = 0, words = 0, errors = 0;
    for (const Size& z : SIZES) {
      if (z.nb == 3 && z.N != 1536) continue;
      std::vector<cf> W, T, ow((size_t)o_fft_twiddle_len(z.N));
      tables(z, W, T);
      o_fft_twiddles(z.N, ow.data());
      if (z.N == 1536 && (memcmp(ow.data(), W.data(), sizeof(cf) * 256) || memcmp(ow.data() + 256, T.data(), sizeof(cf) * 1536))) errors++;
      for (auto& x : inputs(z.N)) {
        std::vector<cf> ref = x, got((size_t)z.N);
        std::vector<int> wr((size_t)z.N, 0);
        o_fft(z.N, ow.data(), ref.data());
        run_schedule(z, x.data(), W.data(), T.data(), got.data(), wr.data(), nullptr, &errors);
        const uint32_t *a = (const uint32_t*)got.data(), *b = (const uint32_t*)ref.data();
        for (int k = 0; k < 2 * z.N; k++) errors += a[k] != b[k];
        cases++; words += 2 * z.N;
      }
    }
    printf("exact: %ld cases %ld words %ld errors\n", cases, words, errors);
    total_errors += errors;
  }
  // ---- three: the restated formula is the oracle's at 1536; the schedule is the restated formula at 384, 768
  {
    long cases = 0, words = 0, errors = 0;
    for (const Size& z : SIZES) {
      if (z.nb != 3) continue;
      const int M = 1 << z.lgM;
      std::vector<cf> W, T;
      tables(z, W, T);
      for (auto& x : inputs(z.N)) {
        std::vector<cf> ref((size_t)z.N), got((size_t)z.N);
        std::vector<int> wr((size_t)z.N, 0);
        three_way(M, W.data(), T.data(), x.data(), ref.data());
        if (z.N == 1536) {
          std::vector<cf> ow((size_t)o_fft_twiddle_len(1536));
          o_fft_twiddles(1536, ow.data());
          got = x;
          o_fft(1536, ow.data(), got.data());
        } else
          run_schedule(z, x.data(), W.data(), T.data(), got.data(), wr.data(), nullptr, &errors);
        errors += memcmp(got.data(), ref.data(), sizeof(cf) * (size_t)z.N) != 0;
        cases++; words += 2 * z.N;
      }
    }
    printf("three: %ld cases %ld words %ld errors\n", cases, words, errors);
    total_errors += errors;
  }
  // ---- bank + cover
  {
    long cover_cases = 0, cover_bins = 0, cover_errors = 0, bank_errors = 0;
    for (const Size& z : SIZES) {
      std::vector<cf> W, T, x((size_t)z.N, cf{0, 0}), got((size_t)z.N);
      tables(z, W, T);
      Trace tr;
      std::vector<int> wr((size_t)z.N, 0);
      run_schedule(z, x.data(), W.data(), T.data(), got.data(), wr.data(), &tr, &cover_errors);
      if (tr.max_slot >= lsn_fft_lds_slots(z.N) || 8 * lsn_fft_lds_slots(z.N) > 12 * z.N) cover_errors++;
      const int nre = nre_of(z.N);
      for (int dc = 0; dc < 2; dc++) {
        std::vector<int> hit((size_t)nre, 0);
        for (int bin = 0; bin < z.N; bin++) {
          const int k = lsn_fft_carrier(bin, z.N, nre, dc);
          if (k < 0) continue;
          if (k >= nre || lsn_fft_carrier_bin(k, z.N, nre, dc) != bin) { cover_errors++; continue; }
          hit[k] += wr[bin];
        }
        for (int k = 0; k < nre; k++) cover_errors += hit[k] != 1;
        cover_cases++; cover_bins += nre;
      }
      long cyc[2] = {0, 0}, extra[2] = {0, 0}, ocyc = 0, oextra = 0;
      int worst[2] = {0, 0}, oworst = 0;
      for (const Access& a : tr.acc) bank_cost(a, &cyc[a.write], &extra[a.write], &worst[a.write]);
      for (const Access& a : old_trace(z, nre, 1).acc) bank_cost(a, &ocyc, &oextra, &oworst);
      if (worst[0] > 1 || worst[1] > 2) bank_errors++;
      printf("bank %d: read %ld cycles %ld extra worst %d, write %ld cycles %ld extra worst %d; before: %ld cycles %ld extra worst %d\n", z.N, cyc[0],
             extra[0], worst[0], cyc[1], extra[1], worst[1], ocyc, oextra, oworst);
    }
    printf("cover: %ld cases %ld words %ld errors\n", cover_cases, cover_bins, cover_errors);
    printf("conflicts: %d cases %d words %ld errors\n", 8, 0, bank_errors);
    total_errors += cover_errors + bank_errors;
  }
  return total_errors ? 1 : 0;
}

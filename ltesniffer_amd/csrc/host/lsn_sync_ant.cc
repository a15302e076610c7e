// lsn_sync_ant.cc - the cell search of lsn_sync.cc over all receive antennas of a recording.  The antennas are combined without their
// phases, per antenna and per 5 ms period: the PSS correlation powers are added (k_pss_corr_ant, kernels/sync_ant.hip), the timing is the peak of that sum, the SSS
// runs per antenna at the common lag (k_sync_fin, unchanged) and the 336 hypothesis powers are added.  With one antenna every number is lsn_cell_search_rates'.
// Product code: no CPU fallback, nothing from oracle/ is included or linked.
#include "lsn_sync_ant.h"
#include "../kernels/lsn_dev.h"
#include "lsn_rates.h"
#include <cmath>
#include <cstring>
#include <vector>

void lsn_launch_sync_fin(const cf32* x, const cf32* p, const cf32* w, const cf32* d, const int8_t* sss, uint32_t N, uint32_t W5, uint32_t P, uint32_t bn,
                         uint32_t cp, void* out, hipStream_t s);

namespace lsn {

void pss_sequence(uint32_t n_id_2, cf32* d);                                  // lsn_sync.cc
void pss_replica_d(uint32_t n_id_2, uint32_t N, double rot_hz, double* p);
void sss_table(uint32_t n_id_2, int8_t* out /* [336][62] */);

namespace {
struct SyncFin {  // LsnSyncFin of stage_sync.hip
  uint32_t j;
  float y[2][2];
  float hyp[336][2];
};
}  // namespace

int cell_search_ant(int device, const cf32* iq, bool on_device, uint64_t nsamples, uint64_t ant_stride, uint32_t A, uint32_t max_ant, uint32_t nof_prb, int rates,
                    const lsn_cell_search_cfg_t& cfg, lsn_cell_search_t& out, lsn_cell_search_ant_t* per_ant, float* corr_out)
{
  std::memset(&out, 0, sizeof out);
  const uint32_t N = symbol_size(nof_prb, rates);  // 0 for an unknown bandwidth or sampling mode: refused below
  const uint32_t P = cfg.nof_periods ? cfg.nof_periods : 1;
  if (!iq || !N || P > 16 || cfg.force_n_id_2 > 2 || cfg.force_n_id_2 < -1) return LSN_ERROR_INVALID_INPUTS;
  const uint32_t W5 = 75 * N;
  const uint64_t need = (uint64_t)(P + 1) * W5 + N;
  if (nsamples < need) return LSN_ERROR_INVALID_INPUTS;
  if (!A || A > max_ant || max_ant > kSearchAntCap || ant_stride < nsamples || ant_stride >= (1ull << 40)) return LSN_ERROR_INVALID_INPUTS;
  if (!have_device(device)) return LSN_ERROR_NO_DEVICE;
  HIP_CHECK(hipSetDevice(device));
  OwnedStream st;

  const uint32_t nroots = cfg.force_n_id_2 >= 0 ? 1u : 3u;
  std::vector<cf32> rep((size_t)nroots * N);
  {
    std::vector<double> pd(2 * (size_t)N);
    for (uint32_t r = 0; r < nroots; r++) {
      pss_replica_d(cfg.force_n_id_2 >= 0 ? (uint32_t)cfg.force_n_id_2 : r, N, 0.0, pd.data());
      for (uint32_t n = 0; n < N; n++) rep[(size_t)r * N + n] = {(float)pd[2 * n], (float)pd[2 * n + 1]};
    }
  }

  DevBuf bx, bp, bc, bk, bw, bd, bs, bo;
  const cf32* d_x = iq;
  size_t astr = (size_t)ant_stride;
  if (!on_device) {  // the part of every antenna the search reads, one after the other
    cf32* dx = bx.alloc<cf32>((size_t)A * need);
    for (uint32_t a = 0; a < A; a++)
      HIP_CHECK(hipMemcpyAsync(dx + (size_t)a * need, iq + (size_t)a * ant_stride, need * sizeof(cf32), hipMemcpyHostToDevice, st));
    d_x = dx;
    astr = (size_t)need;
  }
  cf32* d_p = bp.alloc<cf32>(rep.size());
  float* d_c = bc.alloc<float>((size_t)nroots * W5);
  HIP_CHECK(hipMemcpyAsync(d_p, rep.data(), rep.size() * sizeof(cf32), hipMemcpyHostToDevice, st));
  lsn_launch_pss_corr_ant(d_x, 0, astr, A, d_p, N, W5, P, nroots, 0, W5, d_c, 0, 1, st);
  std::vector<float> C((size_t)nroots * W5);
  HIP_CHECK(hipMemcpyAsync(C.data(), d_c, C.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));

  // cell_search_keep's rule on the combined correlation: first maximum in (root, lag) order; peak over the mean of the winning root
  float best = -1.0f;
  uint32_t br = 0, bn = 0;
  for (uint32_t r = 0; r < nroots; r++)
    for (uint32_t n = 0; n < W5; n++) {
      const float c = C[(size_t)r * W5 + n];
      if (c > best) { best = c; br = r; bn = n; }
    }
  double mean = 0.0;
  for (uint32_t n = 0; n < W5; n++) mean += (double)C[(size_t)br * W5 + n];
  mean /= (double)W5;
  const uint32_t n_id_2 = cfg.force_n_id_2 >= 0 ? (uint32_t)cfg.force_n_id_2 : br;
  if (corr_out) {
    std::memset(corr_out, 0, (size_t)3 * W5 * sizeof(float));
    for (uint32_t r = 0; r < nroots; r++)
      std::memcpy(corr_out + (size_t)(cfg.force_n_id_2 >= 0 ? n_id_2 : r) * W5, C.data() + (size_t)r * W5, (size_t)W5 * sizeof(float));
  }
  out.n_id_2 = n_id_2;
  out.pss_pos = bn;
  out.pss_peak = best;
  out.pss_p2avg = mean > 0.0 ? (float)((double)best / mean) : 0.0f;
  out.found = out.pss_p2avg >= cfg.threshold ? 1u : 0u;

  // every antenna's own share of the peak: the winning root at the common lag, one channel per antenna
  float* d_k = bk.alloc<float>(A);
  lsn_launch_pss_corr_ant(d_x, astr, 0, 1, d_p + (size_t)br * N, N, W5, P, 1, bn, 1, d_k, 1, A, st);
  std::vector<float> own(A);
  HIP_CHECK(hipMemcpyAsync(own.data(), d_k, A * sizeof(float), hipMemcpyDeviceToHost, st));

  // SSS, carrier offset: k_sync_fin per antenna and cyclic-prefix hypothesis at the common lag
  std::vector<cf32> w(N);
  for (uint32_t i = 0; i < N; i++) {
    const double ph = -2.0 * M_PI * (double)i / (double)N;
    w[i] = {(float)std::cos(ph), (float)std::sin(ph)};
  }
  cf32 d[62];
  pss_sequence(n_id_2, d);
  std::vector<int8_t> sss((size_t)336 * 62);
  sss_table(n_id_2, sss.data());
  cf32* d_w = bw.alloc<cf32>(N);
  cf32* d_d = bd.alloc<cf32>(62);
  int8_t* d_s = bs.alloc<int8_t>(sss.size());
  SyncFin* d_o = bo.alloc<SyncFin>((size_t)2 * A);
  HIP_CHECK(hipMemcpyAsync(d_w, w.data(), N * sizeof(cf32), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_d, d, sizeof d, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_s, sss.data(), sss.size(), hipMemcpyHostToDevice, st));
  const uint32_t cps[2] = {144 * N / 2048, 512 * N / 2048};
  for (uint32_t hyp = 0; hyp < 2; hyp++)
    for (uint32_t a = 0; a < A; a++)
      lsn_launch_sync_fin(d_x + (size_t)a * astr, d_p + (size_t)br * N, d_w, d_d, d_s, N, W5, P, bn, cps[hyp], d_o + (size_t)hyp * A + a, st);
  std::vector<SyncFin> fin2((size_t)2 * A);
  HIP_CHECK(hipMemcpyAsync(fin2.data(), d_o, fin2.size() * sizeof(SyncFin), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));

  // The combination.  Every antenna votes in the parity of the FIRST occurrence: hypothesis h of the vote is row h ^ (j & 1) of an antenna whose SSS was taken
  // from occurrence j (subframes 0 and 5 alternate).  M[h] = sum_a |hyp_a[h_a]|^2; the hypotheses are walked in the order of antenna 0's rows, so that one
  // antenna gives lsn_cell_search's walk, ties included.
  float win_m1 = -1.0f;
  for (uint32_t hyp = 0; hyp < 2; hyp++) {
    const SyncFin* fin = &fin2[(size_t)hyp * A];
    const uint32_t cp = cps[hyp];
    float m1 = -1.0f, m2 = -1.0f;
    uint32_t bh = 0;
    for (uint32_t row = 0; row < 336; row++) {
      const uint32_t h = row ^ (fin[0].j & 1u);
      float mt = 0.0f;
      for (uint32_t a = 0; a < A; a++) {
        const float* s = fin[a].hyp[h ^ (fin[a].j & 1u)];
        const float pw = s[0] * s[0] + s[1] * s[1];
        mt = a ? mt + pw : pw;
      }
      if (mt > m1) { m2 = m1; m1 = mt; bh = h; }
      else if (mt > m2) m2 = mt;
    }
    if (!(m1 > win_m1)) continue;   // normal CP on a tie
    win_m1 = m1;
    out.cp = hyp;
    float hr = 0.0f, hi = 0.0f, cr = 0.0f, ci = 0.0f;
    for (uint32_t a = 0; a < A; a++) {
      const SyncFin& f = fin[a];
      const float* s = f.hyp[bh ^ (f.j & 1u)];
      const float r1 = f.y[0][0] * f.y[1][0] + f.y[0][1] * f.y[1][1], i1 = f.y[0][0] * f.y[1][1] - f.y[0][1] * f.y[1][0];  // conj(y0) y1
      hr = a ? hr + s[0] : s[0];
      hi = a ? hi + s[1] : s[1];
      cr = a ? cr + r1 : r1;
      ci = a ? ci + i1 : i1;
    }
    const float cfo_scale = 15000.0f * (float)N / (float)(N + cp);
    out.cfo_coarse_hz = atan2f(ci, cr) / (float)M_PI * 15000.0f;
    out.n_id_1 = bh >> 1;
    out.cell_id = 3 * out.n_id_1 + n_id_2;
    out.sss_metric = m1;
    out.sss_second = m2;
    out.cfo_hz = -atan2f(hi, hr) / (2.0f * (float)M_PI) * cfo_scale;
    const uint32_t pss_off = hyp ? 5 * (N + cp) + cp : 160 * N / 2048 + 6 * (N + cp);
    const uint32_t sf_bn = (bh & 1u) ? 5u : 0u;   // of the first occurrence: the vote's parity
    if (bn >= pss_off) {
      out.sf_start = bn - pss_off;
      out.sf_idx = sf_bn;
    } else {
      out.sf_start = bn + W5 - pss_off;
      out.sf_idx = (sf_bn + 5) % 10;
    }
    if (per_ant)
      for (uint32_t a = 0; a < A; a++) {   // the antenna's own decision under the winning CP hypothesis, by lsn_cell_search's walk over its rows
        const SyncFin& f = fin[a];
        float a1 = -1.0f, a2 = -1.0f, ar = 0.0f, ai = 0.0f;
        uint32_t ah = 0;
        for (uint32_t h = 0; h < 336; h++) {
          const float mt = f.hyp[h][0] * f.hyp[h][0] + f.hyp[h][1] * f.hyp[h][1];
          if (mt > a1) { a2 = a1; a1 = mt; ah = h; ar = f.hyp[h][0]; ai = f.hyp[h][1]; }
          else if (mt > a2) a2 = mt;
        }
        lsn_cell_search_ant_t& o = per_ant[a];
        o.pss_peak = own[a];
        o.sss_metric = a1;
        o.sss_second = a2;
        o.cfo_hz = -atan2f(ai, ar) / (2.0f * (float)M_PI) * cfo_scale;
        o.n_id_1 = ah >> 1;
        o.occurrence = f.j;
      }
  }
  return out.found ? 1 : 0;
}

}  // namespace lsn

extern "C" int lsn_cell_search_ant(int device, const void* iq, int iq_on_device, uint64_t nof_samples, uint64_t ant_stride, uint32_t nof_antennas, uint32_t nof_prb, int rates,
                                   const lsn_cell_search_cfg_t* cfg, lsn_cell_search_t* out, lsn_cell_search_ant_t* per_ant, float* corr_out)
{
  if (!iq || !cfg || !out) return LSN_ERROR_INVALID_INPUTS;
  return lsn::guarded([&]() -> int {
    return lsn::cell_search_ant(device, (const cf32*)iq, iq_on_device != 0, nof_samples, ant_stride, nof_antennas, LSN_SEARCH_MAX_ANTENNAS, nof_prb, rates, *cfg, *out, per_ant,
                                corr_out);
  });
}

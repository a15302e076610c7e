// lsn_sync_all.cc - successive cell search: every cell of a carrier.  Round 0 is lsn_cell_search's decision (cell_search_keep of lsn_sync.cc, which
// leaves its correlation on the device); every round repeats the SSS decision over all occurrences (k_sync_fin_acc), an accepted cell's PSS is cancelled in a
// device copy of the samples (k_pss_cancel) and the correlation is recomputed on the lags the cancellation changed (k_pss_corr_win), maximum and sum per root come
// from k_scan_peaks.  The rule and the patch window are lsn_sync_all.h (no HIP).  Kernels: kernels/cells_sync.hip.  No CPU fallback.
#include "lsn_hip.h"
#include "../kernels/lsn_dev.h"
#include "lsn_clock.h"
#include "lsn_rates.h"
#include "lsn_sync_all.h"
#include <cmath>
#include <cstring>
#include <vector>

void lsn_launch_pss_cancel(cf32* r, const cf32* p, uint32_t N, uint32_t W5, uint32_t P, uint32_t bn, float* a_out, hipStream_t s);
void lsn_launch_pss_corr_win(const cf32* x, const cf32* p, uint32_t N, uint32_t W5, uint32_t P, uint32_t nroots, uint32_t n_lo, uint32_t n_lag, float* C, hipStream_t s);
void lsn_launch_sync_fin_acc(const cf32* x, const cf32* p, const cf32* w, const cf32* d, const int8_t* sss, uint32_t N, uint32_t W5, uint32_t P, uint32_t bn, uint32_t cp0,
                             uint32_t cp1, void* occ, float* acc, hipStream_t s);
void lsn_launch_scan_peaks(const float* C, size_t c_stride, uint32_t W5, uint32_t nroots, uint32_t nch, void* out, hipStream_t s);

namespace lsn {

void pss_sequence(uint32_t n_id_2, cf32* d);                  // lsn_sync.cc
void sss_table(uint32_t n_id_2, int8_t* out /* [336][62] */);
int cell_search_keep(int device, const cf32* iq, bool on_device, uint64_t nsamples, uint32_t nof_prb, int rates, const lsn_cell_search_cfg_t& cfg,
                     lsn_cell_search_t& out, float* corr_out, float* d_corr_keep);

namespace {

struct SyncOcc {  // LsnSyncOcc of cells_sync.hip
  uint32_t valid;
  float y[2][3];
  float hyp[336][2];
};
struct ScanPeak {  // LsnScanPeak of scan.hip
  double sum;
  float peak;
  uint32_t lag;
  uint32_t pad[2];
};

// the replica a cancellation uses: lsn_clock_replica's (double, one rounding)
void rotated_replica(uint32_t n_id_2, uint32_t N, float cfo_hz, std::vector<cf32>& p)
{
  std::vector<double> pd(2 * (size_t)N);
  pss_replica_d(n_id_2, N, (double)cfo_hz, pd.data());
  p.resize(N);
  for (uint32_t n = 0; n < N; n++) p[n] = {(float)pd[2 * n], (float)pd[2 * n + 1]};
}

// the accumulated SSS decision's device side at one (root, lag): tables up, two launches, everything back
struct SssAcc {
  uint32_t N, W5, P;
  DevBuf bp, bw, bd, bs, bo, ba;
  cf32 *d_p = nullptr, *d_w = nullptr, *d_d = nullptr;
  int8_t* d_s = nullptr;
  SyncOcc* d_o = nullptr;
  float* d_a = nullptr;
  std::vector<SyncOcc> occ;
  float acc[2][336];
  uint32_t cps[2];
  int root = -1;

  SssAcc(uint32_t N_, uint32_t W5_, uint32_t P_, hipStream_t st) : N(N_), W5(W5_), P(P_), occ(2 * (size_t)(P_ + 1))
  {
    cps[0] = 144 * N / 2048;
    cps[1] = 512 * N / 2048;
    std::vector<cf32> w(N);
    for (uint32_t i = 0; i < N; i++) {
      const double ph = -2.0 * M_PI * (double)i / (double)N;
      w[i] = {(float)std::cos(ph), (float)std::sin(ph)};
    }
    d_p = bp.alloc<cf32>(N);
    d_w = bw.alloc<cf32>(N);
    d_d = bd.alloc<cf32>(62);
    d_s = bs.alloc<int8_t>((size_t)336 * 62);
    d_o = bo.alloc<SyncOcc>(occ.size());
    d_a = ba.alloc<float>(2 * 336);
    HIP_CHECK(hipMemcpyAsync(d_w, w.data(), N * sizeof(cf32), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));  // w leaves scope
  }
  // unrotated unit-energy replica of the root (float, as lsn_cell_search's), its sequence and its SSS table
  void run(const cf32* d_x, uint32_t n_id_2, const cf32* d_rep /* device, [N] */, uint32_t bn, hipStream_t st)
  {
    if (root != (int)n_id_2) {
      cf32 d[62];
      pss_sequence(n_id_2, d);
      std::vector<int8_t> sss((size_t)336 * 62);
      sss_table(n_id_2, sss.data());
      HIP_CHECK(hipMemcpyAsync(d_d, d, sizeof d, hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(d_s, sss.data(), sss.size(), hipMemcpyHostToDevice, st));
      HIP_CHECK(hipStreamSynchronize(st));
      root = (int)n_id_2;
    }
    lsn_launch_sync_fin_acc(d_x, d_rep, d_w, d_d, d_s, N, W5, P, bn, cps[0], cps[1], d_o, d_a, st);
    HIP_CHECK(hipMemcpyAsync(occ.data(), d_o, occ.size() * sizeof(SyncOcc), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(acc, d_a, sizeof acc, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  // k_sync_fin's choice: the strongest occurrence whose SSS symbol is inside the buffer
  uint32_t strongest(uint32_t cp) const
  {
    uint32_t jb = 0;
    float cjb = -1.0f;
    for (uint32_t j = 0; j <= P; j++) {
      const SyncOcc& o = occ[(size_t)cp * (P + 1) + j];
      if (!o.valid) continue;
      const float sr = o.y[0][0] + o.y[1][0], si = o.y[0][1] + o.y[1][1], et = o.y[0][2] + o.y[1][2];
      const float cj = et > 0.0f ? (sr * sr + si * si) / et : 0.0f;
      if (cj > cjb) { cjb = cj; jb = j; }
    }
    return jb;
  }
};

// a cell from the accumulated decision, by lsn_cell_search's formulas; h: hypothesis at occurrence 0
void fill_cell(const SssAcc& A, uint32_t n_id_2, uint32_t bn, float peak, float p2avg, uint32_t cp_hyp, uint32_t h, float m1, float m2, lsn_cell_search_t& c)
{
  const uint32_t N = A.N, W5 = A.W5, cp = A.cps[cp_hyp];
  const uint32_t jb = A.strongest(cp_hyp);
  const SyncOcc& o = A.occ[(size_t)cp_hyp * (A.P + 1) + jb];
  std::memset(&c, 0, sizeof c);
  c.found = 1;
  c.n_id_2 = n_id_2;
  c.n_id_1 = h >> 1;
  c.cell_id = 3 * c.n_id_1 + n_id_2;
  c.pss_pos = bn;
  c.pss_peak = peak;
  c.pss_p2avg = p2avg;
  c.sss_metric = m1;
  c.sss_second = m2;
  c.cp = cp_hyp;
  {
    const float cr = o.y[0][0] * o.y[1][0] + o.y[0][1] * o.y[1][1], ci = o.y[0][0] * o.y[1][1] - o.y[0][1] * o.y[1][0];  // conj(y0) y1
    c.cfo_coarse_hz = atan2f(ci, cr) / (float)M_PI * 15000.0f;
  }
  const uint32_t hj = h ^ (jb & 1u);  // the same cell's hypothesis at the strongest occurrence
  const float hr = o.hyp[hj][0], hi = o.hyp[hj][1];
  c.cfo_hz = -atan2f(hi, hr) / (2.0f * (float)M_PI) * (15000.0f * (float)N / (float)(N + cp));
  const uint32_t pss_off = cp_hyp ? 5 * (N + cp) + cp : 160 * N / 2048 + 6 * (N + cp);
  const uint32_t sf_bn = (h & 1u) ? 5u : 0u;  // of occurrence 0
  if (bn >= pss_off) {
    c.sf_start = bn - pss_off;
    c.sf_idx = sf_bn;
  } else {
    c.sf_start = bn + W5 - pss_off;
    c.sf_idx = (sf_bn + 5) % 10;
  }
}

double mean_power(const std::vector<float>& a)
{
  double s = 0.0;
  for (size_t j = 0; j + 1 < a.size(); j += 2) s += (double)a[j] * (double)a[j] + (double)a[j + 1] * (double)a[j + 1];
  return a.empty() ? 0.0 : s / (double)(a.size() / 2);
}

int geometry(const void* iq, uint64_t nsamples, uint32_t nof_prb, int rates, uint32_t P, uint32_t& N, uint32_t& W5, uint64_t& need)
{
  N = symbol_size(nof_prb, rates);
  if (!iq || !N || !P || P > 16) return LSN_ERROR_INVALID_INPUTS;
  W5 = 75 * N;
  need = (uint64_t)(P + 1) * W5 + N;
  return nsamples < need ? LSN_ERROR_INVALID_INPUTS : LSN_SUCCESS;
}

int search_all(int device, const cf32* iq, bool on_device, uint64_t nsamples, uint32_t nof_prb, int rates, const lsn_cell_search_all_cfg_t* cfg_in,
               lsn_cell_found_t* out, uint32_t* nof_found, float* corr_out)
{
  CellsCfg cfg;
  if (!out || !nof_found) return LSN_ERROR_INVALID_INPUTS;
  *nof_found = 0;
  const int rc = cells_cfg(cfg_in, cfg);
  if (rc != LSN_SUCCESS) return rc;
  uint32_t N, W5;
  uint64_t need;
  const int rg = geometry(iq, nsamples, nof_prb, rates, cfg.P, N, W5, need);
  if (rg != LSN_SUCCESS) return rg;
  if (!have_device(device)) return LSN_ERROR_NO_DEVICE;
  HIP_CHECK(hipSetDevice(device));
  OwnedStream st;
  const uint32_t P = cfg.P, nroots = cfg.force >= 0 ? 1u : 3u;

  // the working copy: the caller's samples are never written
  DevBuf br_, bc, bq, bpk, bca, ba;
  cf32* d_r = br_.alloc<cf32>(need);
  HIP_CHECK(hipMemcpyAsync(d_r, iq, need * sizeof(cf32), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));
  float* d_c = bc.alloc<float>((size_t)nroots * W5);
  cf32* d_rep = bq.alloc<cf32>((size_t)nroots * N);  // the unrotated replicas, lsn_cell_search's
  {
    std::vector<cf32> rep((size_t)nroots * N), one;
    for (uint32_t r = 0; r < nroots; r++) {
      rotated_replica(cfg.force >= 0 ? (uint32_t)cfg.force : r, N, 0.0f, one);
      std::memcpy(rep.data() + (size_t)r * N, one.data(), N * sizeof(cf32));
    }
    HIP_CHECK(hipMemcpy(d_rep, rep.data(), rep.size() * sizeof(cf32), hipMemcpyHostToDevice));
  }
  ScanPeak* d_pk = bpk.alloc<ScanPeak>(nroots);
  cf32* d_can = bca.alloc<cf32>(N);
  float* d_a = ba.alloc<float>(2 * (size_t)(P + 1));
  SssAcc A(N, W5, P, st);

  // round 0: lsn_cell_search on the untouched samples
  lsn_cell_search_cfg_t c0{P, cfg.force, cfg.threshold};
  lsn_cell_search_t first;
  const int r0 = cell_search_keep(device, d_r, true, need, nof_prb, rates, c0, first, corr_out, d_c);
  if (r0 < 0) return r0;
  if (!first.found) return 0;

  uint32_t nf = 0;
  double pow0 = 0.0;
  for (uint32_t round = 0; nf < cfg.max_cells; round++) {
    uint32_t root = 0, bn = 0;
    float peak = 0.0f;
    double sum = 0.0;
    if (round == 0) {
      root = cfg.force >= 0 ? 0u : first.n_id_2;
      bn = first.pss_pos;
      peak = first.pss_peak;
    } else {
      lsn_launch_scan_peaks(d_c, 0, W5, nroots, 1, d_pk, st);
      ScanPeak pk[3];
      HIP_CHECK(hipMemcpyAsync(pk, d_pk, nroots * sizeof(ScanPeak), hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      float best = -1.0f;
      for (uint32_t r = 0; r < nroots; r++)  // first maximum in (root, lag) order
        if (pk[r].peak > best) { best = pk[r].peak; root = r; }
      bn = pk[root].lag;
      peak = best;
      sum = pk[root].sum;
      if (corr_out) {
        float* co = corr_out + (size_t)round * 3 * W5;
        std::memset(co, 0, (size_t)3 * W5 * sizeof(float));
        if (cfg.force >= 0) HIP_CHECK(hipMemcpy(co + (size_t)cfg.force * W5, d_c, (size_t)W5 * sizeof(float), hipMemcpyDeviceToHost));
        else HIP_CHECK(hipMemcpy(co, d_c, (size_t)3 * W5 * sizeof(float), hipMemcpyDeviceToHost));
      }
    }
    const uint32_t n_id_2 = cfg.force >= 0 ? (uint32_t)cfg.force : root;
    A.run(d_r, n_id_2, d_rep + (size_t)root * N, bn, st);
    lsn_cell_search_all_decision_t dec;  // round 0 was accepted by lsn_cell_search (its p2avg, its sum): only the SSS side of the rule is read there
    cells_decide(cfg, round, peak, round ? sum : 1.0, round ? W5 : 1u, &A.acc[0][0], &dec);
    lsn_cell_found_t f;
    std::memset(&f, 0, sizeof f);
    if (round == 0) {
      f.cell = first;  // lsn_cell_search's answer, field by field
    } else {
      if (!dec.accept) break;
      fill_cell(A, n_id_2, bn, peak, dec.p2avg, dec.cp, dec.best, dec.best_power, dec.second_power, f.cell);
      bool seen = false;
      for (uint32_t i = 0; i < nf; i++) seen = seen || out[i].cell.cell_id == f.cell.cell_id;
      if (seen) break;  // what a cancellation left of a cell is not a new cell
    }
    f.round = round;
    f.sss_ratio = dec.sss_ratio;

    // cancel; the gains are the cell's relative power
    std::vector<cf32> rot;
    rotated_replica(n_id_2, N, f.cell.cfo_hz, rot);
    HIP_CHECK(hipMemcpyAsync(d_can, rot.data(), N * sizeof(cf32), hipMemcpyHostToDevice, st));
    lsn_launch_pss_cancel(d_r, d_can, N, W5, P, bn, d_a, st);
    std::vector<float> a(2 * (size_t)(P + 1));
    HIP_CHECK(hipMemcpyAsync(a.data(), d_a, a.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const double pw = mean_power(a);
    if (round == 0) pow0 = pw;
    f.rel_power_db = pw > 0.0 && pow0 > 0.0 ? (float)(10.0 * std::log10(pw / pow0)) : 0.0f;
    out[nf++] = f;

    if (dec.shared && nf < cfg.max_cells) {
      lsn_cell_found_t g;
      std::memset(&g, 0, sizeof g);
      // round 0 keeps lsn_cell_search's CP for cell 0; its twin is read from the accumulated decision's winning CP
      fill_cell(A, n_id_2, bn, peak, f.cell.pss_p2avg, dec.cp, dec.runner_up, dec.runner_up_power, dec.best_power, g.cell);
      bool seen = false;
      for (uint32_t i = 0; i < nf; i++) seen = seen || out[i].cell.cell_id == g.cell.cell_id;
      if (!seen) {
        g.round = round;
        g.shared_pss = 1;
        g.sss_ratio = dec.sss_ratio;
        g.rel_power_db = f.rel_power_db + (float)(10.0 * std::log10((double)dec.runner_up_power / (double)dec.best_power));
        out[nf++] = g;
      }
    }
    if (nf >= cfg.max_cells) break;

    lsn_cell_search_all_plan_t pl;
    cells_plan(bn, N, W5, &pl);
    for (uint32_t i = 0; i < pl.nof_runs; i++) lsn_launch_pss_corr_win(d_r, d_rep, N, W5, P, nroots, pl.run_lo[i], pl.run_len[i], d_c, st);
  }
  HIP_CHECK(hipStreamSynchronize(st));
  *nof_found = nf;
  return (int)nf;
}

}  // namespace
}  // namespace lsn

extern "C" {

int lsn_cell_search_all(int device, const void* iq, int iq_on_device, uint64_t nof_samples, uint32_t nof_prb, int rates, const lsn_cell_search_all_cfg_t* cfg,
                        lsn_cell_found_t* out, uint32_t* nof_found, float* corr_out)
{
  return lsn::guarded([&]() -> int { return lsn::search_all(device, (const cf32*)iq, iq_on_device != 0, nof_samples, nof_prb, rates, cfg, out, nof_found, corr_out); });
}

int lsn_pss_cancel(int device, const void* iq, uint64_t nof_samples, uint32_t nof_prb, int rates, uint32_t nof_periods, uint32_t n_id_2, uint32_t pss_pos,
                   float cfo_hz, void* residual, float* a_out)
{
  return lsn::guarded([&]() -> int {
    uint32_t N, W5;
    uint64_t need;
    const int rg = lsn::geometry(iq, nof_samples, nof_prb, rates, nof_periods, N, W5, need);
    if (rg != LSN_SUCCESS) return rg;
    if (!residual || !a_out || n_id_2 > 2 || pss_pos >= W5 || !std::isfinite(cfo_hz)) return LSN_ERROR_INVALID_INPUTS;
    if (!lsn::have_device(device)) return LSN_ERROR_NO_DEVICE;
    HIP_CHECK(hipSetDevice(device));
    lsn::OwnedStream st;
    lsn::DevBuf bx, bp, ba;
    cf32* d_r = bx.alloc<cf32>(nof_samples);
    cf32* d_p = bp.alloc<cf32>(N);
    float* d_a = ba.alloc<float>(2 * (size_t)(nof_periods + 1));
    std::vector<cf32> rot;
    lsn::rotated_replica(n_id_2, N, cfo_hz, rot);
    HIP_CHECK(hipMemcpyAsync(d_r, iq, nof_samples * sizeof(cf32), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_p, rot.data(), N * sizeof(cf32), hipMemcpyHostToDevice, st));
    lsn_launch_pss_cancel(d_r, d_p, N, W5, nof_periods, pss_pos, d_a, st);
    HIP_CHECK(hipMemcpyAsync(residual, d_r, nof_samples * sizeof(cf32), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(a_out, d_a, 2 * (size_t)(nof_periods + 1) * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return LSN_SUCCESS;
  });
}

int lsn_sss_accumulate(int device, const void* iq, uint64_t nof_samples, uint32_t nof_prb, int rates, uint32_t nof_periods, uint32_t n_id_2, uint32_t pss_pos,
                       float* sums, uint32_t* valid, float* halves, float* acc)
{
  return lsn::guarded([&]() -> int {
    uint32_t N, W5;
    uint64_t need;
    const int rg = lsn::geometry(iq, nof_samples, nof_prb, rates, nof_periods, N, W5, need);
    if (rg != LSN_SUCCESS) return rg;
    if (!sums || !valid || !halves || !acc || n_id_2 > 2 || pss_pos >= W5) return LSN_ERROR_INVALID_INPUTS;
    if (!lsn::have_device(device)) return LSN_ERROR_NO_DEVICE;
    HIP_CHECK(hipSetDevice(device));
    lsn::OwnedStream st;
    lsn::DevBuf bx, bp;
    cf32* d_x = bx.alloc<cf32>(need);
    cf32* d_p = bp.alloc<cf32>(N);
    std::vector<cf32> rep;
    lsn::rotated_replica(n_id_2, N, 0.0f, rep);
    HIP_CHECK(hipMemcpyAsync(d_x, iq, need * sizeof(cf32), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_p, rep.data(), N * sizeof(cf32), hipMemcpyHostToDevice, st));
    lsn::SssAcc A(N, W5, nof_periods, st);
    A.run(d_x, n_id_2, d_p, pss_pos, st);
    const uint32_t nocc = nof_periods + 1;
    for (uint32_t c = 0; c < 2; c++)
      for (uint32_t j = 0; j < nocc; j++) {
        const lsn::SyncOcc& o = A.occ[(size_t)c * nocc + j];
        valid[c * nocc + j] = o.valid;
        float* s = sums + ((size_t)c * nocc + j) * 336 * 2;
        if (o.valid) std::memcpy(s, o.hyp, sizeof o.hyp);
        else std::memset(s, 0, sizeof o.hyp);
      }
    {  // the halves do not depend on the CP; an occurrence is evaluated under the normal CP whenever it is under the extended one
      for (uint32_t j = 0; j < nocc; j++) {
        const lsn::SyncOcc& o = A.occ[j];
        if (o.valid) std::memcpy(halves + (size_t)j * 6, o.y, sizeof o.y);
        else std::memset(halves + (size_t)j * 6, 0, sizeof o.y);
      }
    }
    std::memcpy(acc, A.acc, sizeof A.acc);
    return LSN_SUCCESS;
  });
}

int lsn_cell_search_all_plan(uint32_t pss_pos, uint32_t N, uint32_t W5, lsn_cell_search_all_plan_t* out) { return lsn::cells_plan(pss_pos, N, W5, out); }

int lsn_cell_search_all_decide(const lsn_cell_search_all_cfg_t* cfg, uint32_t round, float peak, double sum, uint32_t W5, const float* acc,
                               lsn_cell_search_all_decision_t* out)
{
  lsn::CellsCfg c;
  const int rc = lsn::cells_cfg(cfg, c);
  if (rc != LSN_SUCCESS) return rc;
  return lsn::cells_decide(c, round, peak, sum, W5, acc, out);
}

}  // extern "C"

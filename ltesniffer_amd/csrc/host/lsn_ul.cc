// lsn_ul.cc - uplink half of the engine: cell-constant uplink tables and the batched PUSCH grant decoder
// (srsran_enb_ul_fft + srsran_chest_ul_estimate_pusch + srsran_pusch_decode for a list of grants,
// /root/reference/src/src/UL_Sniffer_PUSCH.cc:250-262,389-392).  The UL-mode orchestration around it (ULSchedule,
// modulation-table trials, Msg3 grants) is host logic that calls this entry point.
// Product code: no CPU fallback, nothing from oracle/ is included or linked.
#include "lsn_engine.h"
#include "../kernels/lsn_rm.h"
#include "../../../spec/lte_tables.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

namespace lsn {

static int largest_prime_below(int n)
{
  for (int p = n - 1; p >= 2; p--) {
    bool ok = true;
    for (int d = 2; d * d <= p; d++)
      if (p % d == 0) { ok = false; break; }
    if (ok) return p;
  }
  return 2;
}

template <typename T>
static T* upload_vec(std::vector<void*>& allocs, const std::vector<T>& v)
{
  void* d = nullptr;
  HIP_CHECK(hipMalloc(&d, v.size() * sizeof(T) + 16));
  HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  allocs.push_back(d);
  return (T*)d;
}

// 7.5 kHz shift of the SC-FDMA demodulator: needed by the uplink OFDM stage of every chunk, also before SIB2 is known
void Engine::uploadUlStatic()
{
  if (cd.ul_shift) return;
  const int N = (int)cd.N;
  std::vector<cf32> sh((size_t)N);
  for (int n = 0; n < N; n++) { const double a = M_PI * n / N; sh[n] = {(float)std::cos(a), (float)(-std::sin(a))}; }
  cd.ul_shift = upload_vec(dev_allocs, sh);
}

bool Engine::getUlConfig(lsn_ul_cfg_t* u, lsn_prach_cfg_t* p, Sib2Config* sib) const
{
  if (!ul_set) return false;
  if (u) *u = ul_cfg;
  if (p) { *p = prach.cfg; if (!prach.set) p->config_idx = 0xFFFFFFFFu; }
  if (sib) *sib = sib2;
  return true;
}

// srsran_enb_ul_set_cell with the DMRS configuration of SIB2 (SubframeWorker.cc:258-262, ULSchedule.cc:140-158): the configuration becomes the
// shared one (every engine of a multi-GPU capture follows it, syncUlConfig), this engine's device tables are built now
int Engine::setUlConfig(const lsn_ul_cfg_t& u)
{
  if (!cell_set || u.cyclic_shift > 7 || u.delta_ss > 29) return LSN_ERROR_INVALID_INPUTS;
  const int r = buildUlTables(u);
  if (r != LSN_SUCCESS) return r;
  ul_cfg = u;
  ul_set = true;
  sib2_learned = false;
  ul_tables_epoch = ul_cfg_epoch.fetch_add(1, std::memory_order_release) + 1;
  return LSN_SUCCESS;
}

// commit turn of an UL_MODE chunk: another engine of the capture (or the caller, through engine 0) may have (re)configured the uplink since this
// engine built its tables
void Engine::syncUlConfig()
{
  const uint32_t ep = ul_cfg_epoch.load(std::memory_order_acquire);
  if (ul_set && ul_tables_epoch != ep) {
    if (buildUlTables(ul_cfg) != LSN_SUCCESS) throw std::runtime_error("UL_MODE: the shared uplink configuration could not be applied on this device");
    ul_tables_epoch = ep;
  }
  if (sh->prach_cfg_set && prach_tables_epoch != sh->prach_epoch) {
    const uint32_t pe = sh->prach_epoch;
    const lsn_prach_cfg_t pc = sh->prach_cfg;
    if (setPrachConfig(pc) != LSN_SUCCESS) prach.set = false;
    sh->prach_epoch = pe;          // (setPrachConfig counted a new epoch: this was a replay of the shared one)
    prach_tables_epoch = pe;
  }
}

int Engine::buildUlTables(const lsn_ul_cfg_t& u)
{
  if (!cell_set || u.cyclic_shift > 7 || u.delta_ss > 29) return LSN_ERROR_INVALID_INPUTS;
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(cfg.device));
    const int N = (int)cd.N;
    (void)N;
    std::vector<cf32> ph(12), base, idft;
    for (int m = 0; m < 12; m++) { const double a = 2.0 * M_PI * m / 12.0; ph[m] = {(float)std::cos(a), (float)std::sin(a)}; }
    const uint32_t fss = ((cell.id % 30u) + u.delta_ss) % 30u;  // f_ss^PUSCH
    // Base sequences r_{u,v}(n) of every allocation size for all 30 sequence groups and both sequence numbers (36.211 5.5.1.1 / 5.5.1.2):
    // variant (2 u + v) of size L starts at (2 u + v) * ul_base_stride + ul_off[L]; v = 1 only exists from 6 PRB on (else a copy of v = 0).
    ul_off.assign(111, -1);
    uint32_t stride = 0;
    for (uint32_t L = 1; L <= cell.nof_prb; L++) {
      if (!ul_valid_prb(L)) continue;
      ul_off[L] = (int)stride; stride += 12 * L;
    }
    ul_base_stride = stride;
    base.resize((size_t)60 * stride);
    for (uint32_t L = 1; L <= cell.nof_prb; L++) {
      if (ul_off[L] < 0) continue;
      const int M = 12 * (int)L, Nzc = largest_prime_below(M);
      for (uint32_t uu = 0; uu < 30; uu++)
        for (uint32_t vv = 0; vv < 2; vv++) {
          cf32* dst = base.data() + (size_t)(2 * uu + vv) * stride + ul_off[L];
          const double qb = (double)Nzc * (double)(uu + 1) / 31.0;
          long long q = (long long)std::floor(qb + 0.5);
          if (vv && M >= 72) q += ((long long)std::floor(2.0 * qb) & 1) ? -1 : 1;
          for (int n = 0; n < M; n++) {
            if (L <= 2) {  // one / two PRB: the tabulated sequences exp(j phi(n) pi / 4) (Tables 5.5.1.2-1 / -2, spec/lte_tables.h)
              const double a = M_PI * (double)(L == 1 ? lsn_dmrs_phi12[uu][n] : lsn_dmrs_phi24[uu][n]) / 4.0;
              dst[n] = {(float)std::cos(a), (float)std::sin(a)};
              continue;
            }
            const long long m = n % Nzc;
            const double a = M_PI * (double)((q * m * (m + 1)) % (2ll * Nzc)) / (double)Nzc;
            dst[n] = {(float)std::cos(a), (float)(-std::sin(a))};
          }
        }
      for (int k = 0; k < M; k++) { const double a = 2.0 * M_PI * k / M; idft.push_back({(float)std::cos(a), (float)std::sin(a)}); }
    }
    // sequence group u(ns) and sequence number v(ns) of the 20 slots (5.5.1.3 / 5.5.1.4)
    {
      std::vector<uint8_t> cg(8 * 20 + 8), cs(32);
      gold_sequence(cell.id / 30u, cg.data(), 8 * 20);
      gold_sequence(((cell.id / 30u) << 5) + fss, cs.data(), 20);
      for (uint32_t ns = 0; ns < 20; ns++) {
        uint32_t fgh = 0;
        if (u.group_hopping_enabled) { for (int i = 0; i < 8; i++) fgh += (uint32_t)cg[8 * ns + i] << i; fgh %= 30u; }
        ul_u[ns] = (uint8_t)((fgh + fss) % 30u);
        ul_v[ns] = (uint8_t)((!u.group_hopping_enabled && u.sequence_hopping_enabled) ? cs[ns] : 0);
      }
    }
    uploadUlStatic();
    cd.ul_ph12 = upload_vec(dev_allocs, ph);
    cd.ul_base = upload_vec(dev_allocs, base);
    cd.ul_idft = upload_vec(dev_allocs, idft);
    // n_PN(ns) of 36.211 5.5.2.1.1
    std::vector<uint8_t> c(8 * 7 * 20 + 8);
    gold_sequence(((cell.id / 30u) << 5) + fss, c.data(), (int)c.size());
    for (uint32_t ns = 0; ns < 20; ns++) {
      uint32_t npn = 0;
      for (int i = 0; i < 8; i++) npn += (uint32_t)c[8 * (int)cell.nslot() * ns + i] << i;   // n_PN(ns) = sum c(8 N_symb^UL ns + i) 2^i (36.211 5.5.2.1.1)
      ul_npn[ns] = npn;
    }
    cell.pusch_hop_offset = u.hopping_offset;  // n_rb_ho of the DCI 0 -> grant conversion from now on (SubframeWorker.cc:271-277)
    search->setPuschHopOffset(u.hopping_offset);
    if (!runner_u.stream) allocRunner(runner_u);
    return LSN_SUCCESS;
  });
}

int Engine::puschDecode(const void* ul_iq, bool on_device, uint32_t nsf, uint32_t start_tti, const lsn_pusch_grant_t* grants, uint32_t ngrants,
                        lsn_pusch_result_t* results, uint8_t* payloads, size_t payload_cap)
{
  if (!cell_set || !ul_set) return LSN_ERROR;
  if ((!ul_iq && nsf) || (!grants && ngrants) || (!results && ngrants)) return LSN_ERROR_INVALID_INPUTS;
  return guarded([&]() -> int {
    HIP_CHECK(hipSetDevice(cfg.device));
    hipStream_t st = runner_u.stream;   // the one stream that touches ul_d_iq and ul_d_grid (prachDetect's copy into ul_d_iq is on it as well): grow_dev waits for it alone
    const cf32* d_iq = (const cf32*)ul_iq;
    if (!on_device) {
      grow_dev(ul_d_iq, ul_iq_cap, (size_t)nsf * cd.sflen, st);
      HIP_CHECK(hipMemcpyAsync(ul_d_iq, ul_iq, (size_t)nsf * cd.sflen * sizeof(cf32), hipMemcpyHostToDevice, st));
      d_iq = ul_d_iq;
    }
    grow_dev(ul_d_grid, ul_grid_cap, (size_t)nsf * 14 * cd.nre, st);
    lsn_launch_ul_fft(cd, d_iq, 1, 0, ul_d_grid, nsf, st);
    std::vector<uint8_t> pay;
    puschDecodeGrid(ul_d_grid, nsf, start_tti, grants, ngrants, results, pay, d_iq, 1, 0);
    if (payloads && pay.size() > payload_cap) return LSN_ERROR_INVALID_INPUTS;  // results[].payload_off would point past the caller's buffer
    if (payloads) std::memcpy(payloads, pay.data(), pay.size());
    return LSN_SUCCESS;
  });
}

// srsran_chest_ul_estimate_pusch + srsran_pusch_decode for a list of grants on an uplink grid that is already on the device
// (stream runner_u).  payload_out: tbs/8 bytes per valid grant at results[i].payload_off.  Throws on HIP errors.
// With lsn_phy_set_ul_timing (mode 1 / 2) k_pusch_toa measures every grant's arrival on d_grid and decides its window shift; in mode 2, given the samples
// (d_src), k_ul_fft_win cuts the grants again into private rows, the estimate and the demodulator run on those, and k_pusch_toa once more for the
// residual.  No host wait between the passes.  timing (optional): one record per caller's grant.
void Engine::puschDecodeGrid(const cf32* d_grid, uint32_t nsf, uint32_t start_tti, const lsn_pusch_grant_t* grants, uint32_t ngrants,
                             lsn_pusch_result_t* results, std::vector<uint8_t>& payload_out, const cf32* d_src, uint32_t src_nant, uint32_t src_ant,
                             lsn_pusch_timing_t* timing)
{
  static const uint32_t n_dmrs1[8] = {0, 2, 3, 4, 6, 8, 9, 10};  // 36.211 Table 5.5.2.1.1-2
  static const uint32_t n_dmrs2[8] = {0, 6, 3, 4, 2, 8, 10, 9};  // Table 5.5.2.1.1-1
  JobRunner& r = runner_u;
  hipStream_t st = r.stream;
  payload_out.clear();
  std::vector<LsnUlGrantDev> gd;
  std::vector<int> gidx;
  r.h_cbs.clear();
  struct TbRef { uint32_t grant, cb_first, cb_count, pay_off; int tbs; };
  std::vector<TbRef> tbs;
  size_t hs_n = 0, llr_n = 0, pay_n = 0;
  for (uint32_t i = 0; i < ngrants; i++) {
    const lsn_pusch_grant_t& g = grants[i];
    results[i] = lsn_pusch_result_t{};
    const uint32_t n_prb2 = g.hop == 1 ? g.n_prb_slot1 : g.n_prb;
    // (no uint32 wrap-around in the range checks: n_prb <= nof_prb first, then L_prb against what is left)
    const bool ok = g.sf < nsf && g.L_prb >= 1 && g.L_prb <= cell.nof_prb && ul_valid_prb(g.L_prb) && g.n_prb <= cell.nof_prb - g.L_prb && n_prb2 <= cell.nof_prb - g.L_prb && g.hop <= 1 &&
                    g.tbs > 0 && (g.tbs % 8) == 0 &&
                    (g.mod == 2 || g.mod == 4 || g.mod == 6 || g.mod == 8) && ul_off[g.L_prb] >= 0 && g.rv >= 0 && g.rv < 4;
    if (!ok) continue;
    const uint32_t M = 12 * g.L_prb, sf_idx = (start_tti + g.sf) % 10;
    const uint32_t C = 2 * (cell.nslot() - 1);  // N_symb^PUSCH: 12 SC-FDMA data symbols per subframe, 10 with the extended CP (= columns of the channel interleaver)
    CbSegm s;
    if (!cbsegm((int)g.tbs, s)) continue;
    // control resources Q' = min(ceil(O M_sc N_symb beta / sum K_r), cap) (36.212 5.2.2.6), beta in eighths
    const long long sumK = (long long)s.Cp * s.Kp + (long long)s.Cm * s.Km;
    auto qprime = [&](uint32_t O, long long beta8, uint32_t cap) -> uint32_t {
      if (!O) return 0u;
      const long long q = ((long long)O * M * C * beta8 + 8 * sumK - 1) / (8 * sumK);
      return (uint32_t)std::min<long long>(q, cap);
    };
    if (g.nof_ack > 2 || g.ri_bits > 2 || g.cqi_bits > 64) continue;
    // beta offsets of the UE (36.213 Tables 8.6.3-1/-2/-3, spec/lte_tables.h), the reference's defaults when the grant does not name them
    const uint32_t ia = g.beta_offset_ack_idx_p1 ? g.beta_offset_ack_idx_p1 - 1 : 10u, ic = g.beta_offset_cqi_idx_p1 ? g.beta_offset_cqi_idx_p1 - 1 : 8u,
                   ir = g.beta_offset_ri_idx_p1 ? g.beta_offset_ri_idx_p1 - 1 : 11u;
    if (ia > 15 || ic > 15 || ir > 15) continue;
    if ((g.nof_ack && !lsn_beta_ack8[ia]) || (g.ri_bits && !lsn_beta_ri8[ir]) || (g.cqi_bits && !lsn_beta_cqi8[ic])) continue;  // reserved index
    const uint32_t q_ack = qprime(g.nof_ack, lsn_beta_ack8[ia], 4 * M), q_ri = qprime(g.ri_bits, lsn_beta_ri8[ir], 4 * M);
    const uint32_t q_cqi = g.cqi_bits ? qprime(g.cqi_bits + (g.cqi_bits > 11 ? 8u : 0u), lsn_beta_cqi8[ic], C * M - q_ri) : 0u;
    if (q_ri + q_cqi >= C * M) continue;
    const int G = (int)((C * M - q_ri - q_cqi) * g.mod);
    LsnUlGrantDev d{};
    d.sf = g.sf; d.n_prb = g.n_prb; d.n_prb2 = n_prb2; d.L_prb = g.L_prb; d.qm = g.mod;
    for (uint32_t sl = 0; sl < 2; sl++) d.ncs[sl] = (n_dmrs1[ul_cfg.cyclic_shift & 7] + n_dmrs2[g.n_dmrs & 7] + ul_npn[2 * sf_idx + sl]) % 12u;
    d.cinit = ((uint32_t)g.rnti << 14) | (sf_idx << 9) | cell.id;
    for (uint32_t sl = 0; sl < 2; sl++) {
      const uint32_t ns = 2 * sf_idx + sl, var = 2u * ul_u[ns] + (g.L_prb >= 6 ? ul_v[ns] : 0u);
      (sl ? d.base_off1 : d.base_off) = var * ul_base_stride + (uint32_t)ul_off[g.L_prb];
    }
    d.idft_off = (uint32_t)ul_off[g.L_prb];
    d.hs_off = (uint32_t)hs_n; hs_n += 2 * M;
    d.llr_off = (uint32_t)llr_n; llr_n += ((size_t)G + 7) & ~(size_t)7;
    d.scale = 1.0f / sqrtf((float)M);
    d.q_ack = q_ack; d.q_ri = q_ri; d.q_cqi = q_cqi;
    // UL-SCH: one transport block, one layer (36.212 5.2.2.6)
    TbRef ref{i, (uint32_t)r.h_cbs.size(), (uint32_t)s.C, (uint32_t)pay_n, (int)g.tbs};
    // no skipping behind a failed block 0: every code block is decoded, the iteration count of a grant is part of what lsn_phy_pusch_decode reports
    pay_n += tb_code_blocks(s, G, (int)g.mod, 1, g.rv, (uint32_t)cfg.max_turbo_iterations, d.llr_off, (uint32_t)pay_n, false, r.h_cbs);
    tbs.push_back(ref);
    gd.push_back(d);
    gidx.push_back((int)i);
  }
  ul_last_gd = gd; ul_last_idx = gidx;
  ul_last_cbs.clear(); ul_last_tbs.clear();
  const uint32_t tmode = ul_timing.mode;
  const bool rewin = tmode == 2 && d_src;
  ul_last_timing.assign(ngrants, lsn_pusch_timing_t{}); ul_last_priv = false;
  if (timing) std::fill(timing, timing + ngrants, lsn_pusch_timing_t{});
  const uint32_t ng = (uint32_t)gd.size(), ncb = (uint32_t)r.h_cbs.size();
  if (!ng) { HIP_CHECK(hipStreamSynchronize(st)); return; }
  // (these arenas are runner_u's, written and read on its stream only - also when the UL_MODE commit calls in with a chunk's grid, which stage A finished long ago)
  grow_dev(ul_d_grants, ul_grants_cap, ng, st);
  grow_dev(ul_d_hs, ul_hs_cap, hs_n, st);
  grow_dev(ul_d_stat, ul_stat_cap, (size_t)2 * ng, st);
  grow_dev(r.d_llr16, r.llr16_cap, llr_n + 8, st);
  grow_dev(r.d_cbs, r.cbs_cap, ncb, st);
  grow_dev(r.d_cbres, r.cbres_cap, ncb, st);
  grow_dev(r.d_payload, r.payload_cap, pay_n + 16, st);
  if (tmode) { grow_dev(ul_d_toa, ul_toa_cap, ng, st); grow_host(ul_h_toa, ul_h_toa_cap, ng, st); }
  if (rewin) { grow_dev(ul_d_grants2, ul_grants2_cap, ng, st); grow_dev(ul_d_priv, ul_priv_cap, (size_t)ng * 14 * cd.nre, st); }
  const TurboOrder to = turbo_classic_order(r.h_cbs);
  // descriptors go through pinned mirrors and the upload kernel, not through the host -> device copy engine (its FIFO may hold IQ blocks, lsn_dev.h)
  grow_host(ul_h_grants, ul_h_grants_cap, ng, st);
  grow_host(r.h_cbs_pinned, r.h_cbs_cap, ncb, st);
  const TurboPlacement place = turbo_place(r.h_cbs, to.order, 0, r.h_cbs_pinned);
  grow_dev(r.d_spp, r.spp_cap, place.spp_n + 16, st);
  std::memcpy(ul_h_grants, gd.data(), ng * sizeof(LsnUlGrantDev));
  lsn_launch_upload(ul_d_grants, ul_h_grants, ng * sizeof(LsnUlGrantDev), st);
  lsn_launch_upload(r.d_cbs, r.h_cbs_pinned, ncb * sizeof(LsnCbDev), st);
  HIP_CHECK(hipMemsetAsync(r.d_llr16, 0, llr_n * sizeof(int16_t), st));
  const LsnUlGrantDev* d_g = ul_d_grants;   // what the estimate and the demodulator read: the common grid, or in mode 2 every grant's private rows
  const cf32* d_rows = d_grid;
  const LsnUlToaCfg tc = ulToaCfg();
  if (tmode) lsn_launch_pusch_toa(cd, ul_d_grants, d_grid, tc, ul_d_toa, ul_h_toa, rewin ? ul_d_grants2 : nullptr, false, ng, st);
  if (rewin) {
    lsn_launch_ul_fft_win(cd, d_src, src_nant, src_ant, ul_d_grants, ul_d_toa, d_grid, ul_d_priv, ng, st);
    d_g = ul_d_grants2; d_rows = ul_d_priv;
    ul_last_priv = true;
  }
  lsn_launch_pusch_chest(cd, d_g, d_rows, ul_d_hs, ul_d_stat, ng, st);
  lsn_launch_pusch_demod(cd, d_g, d_rows, ul_d_hs, ul_d_stat, r.d_llr16, ng, st);
  if (rewin) lsn_launch_pusch_toa(cd, d_g, d_rows, tc, ul_d_toa, ul_h_toa, nullptr, true, ng, st);
  lsn_launch_rm(r.d_cbs, r.d_llr16, r.d_spp, ncb, place.emax, st);
  lsn_launch_turbo(cd, r.d_cbs, r.d_spp, r.d_payload, r.d_cbres, to.n128, to.kmax128, ncb - to.n128, to.kmax64, st);
  // results come back through pinned mirrors written by the copy kernel (lsn_dev.h), not through the copy engine
  grow_host(r.h_cbres_pinned, r.h_cbres_cap, ncb, st);
  grow_host(r.h_payload_pinned, r.h_payload_cap, pay_n + 16, st);
  grow_host(ul_h_stat, ul_h_stat_cap, (size_t)2 * ng, st);
  lsn_launch_download(r.h_cbres_pinned, r.d_cbres, ncb * sizeof(LsnCbRes), st);
  lsn_launch_download(r.h_payload_pinned, r.d_payload, pay_n, st);
  lsn_launch_download(ul_h_stat, ul_d_stat, (size_t)2 * ng * sizeof(float), st);
  HIP_CHECK(hipStreamSynchronize(st));
  const LsnCbRes* cbres = r.h_cbres_pinned;
  const uint8_t* pay_base = r.h_payload_pinned;
  const float* stat = ul_h_stat;
  for (size_t t = 0; t < tbs.size(); t++) {
    const TbRef& ref = tbs[t];
    const TbResult tr = tb_verdict(cbres + ref.cb_first, r.h_cbs.data() + ref.cb_first, ref.cb_count);
    const uint8_t* pl = pay_base + ref.pay_off;
    lsn_pusch_result_t& res = results[ref.grant];
    res.crc_ok = tr.v.pass(pl, ref.tbs);
    res.iterations = tr.iters;
    res.snr_db = 10.0f * log10f(stat[2 * t + 1] / stat[2 * t]);
    res.payload_off = (uint32_t)payload_out.size();
    payload_out.insert(payload_out.end(), pl, pl + ref.tbs / 8);
    if (tmode) {  // (k_pusch_toa wrote the pinned mirror; tbs[t] belongs to gd[t])
      const LsnUlToaDev& q = ul_h_toa[t];
      lsn_pusch_timing_t& o = ul_last_timing[ref.grant];
      o.measured = 1; o.tau = q.tau; o.shift = q.shift; o.flags = q.flags; o.residual = q.residual; o.confidence = q.conf;
      o.toa_us = (rewin ? (float)q.shift + q.residual : q.tau) * (1.0e6f / (15000.0f * (float)cd.N));
      if (timing) timing[ref.grant] = o;
    }
  }
  // taps 3 / 4: the blocks of every grant in transport-block order with their verdicts and where turbo_place put their de-rate-matched words (tbs[t] belongs to gd[t])
  ul_last_cbs.reserve(ncb);
  for (const TbRef& ref : tbs) {
    ul_last_tbs.push_back({(uint32_t)ul_last_cbs.size(), ref.cb_count});
    for (uint32_t q = ref.cb_first; q < ref.cb_first + ref.cb_count; q++) {
      const LsnCbDev& cb = r.h_cbs[q];
      const LsnCbRes& cr = cbres[cb.res_idx];
      ul_last_cbs.push_back({cb.K, cb.F, cb.E, cb.rv, cr.ok, cr.iters, place.spp_of[q]});
    }
  }
}

LsnUlToaCfg Engine::ulToaCfg() const
{
  const int32_t N = (int32_t)cd.N;
  LsnUlToaCfg c;
  c.min_shift = ul_timing.min_shift ? (int32_t)ul_timing.min_shift : std::max(1, N / 128);
  c.max_advance = ul_timing.max_advance ? (int32_t)ul_timing.max_advance : N / 4;
  c.late_max = 144 * N / 2048;
  return c;
}

int Engine::setUlTiming(const lsn_ul_timing_cfg_t& t)
{
  if (!cell_set || batch_open) return LSN_ERROR;  // the thresholds are in samples of the cell; not while submitted blocks are in flight (call lsn_phy_wait first)
  if (t.mode > 2 || t.max_advance > cd.N / 2 || t.min_shift > cd.N / 2) return LSN_ERROR_INVALID_INPUTS;
  ul_timing = t;
  return LSN_SUCCESS;
}

// the row of the reference's uplink table (MCSTracking.cc:441-472) for one RNTI; the sums are kept where update_statistic_ul is restated (lsn_ulmode.cc)
int Engine::getUlUeStats(uint16_t rnti, lsn_ul_ue_stats_t* out)
{
  if (cfg.sniffer_mode != 1) return LSN_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lk(mcs_mtx);
  *out = lsn_ul_ue_stats_t{};
  if (ulmod.empty() || !ulmod[rnti]) return 0;
  out->mod = ulmod[rnti]; out->active = ul_active[rnti]; out->success = ul_success[rnti];
  if (out->active) out->mean_snr_db = ul_snr_sum[rnti] / (float)out->active;
  out->measured = ul_toa_n[rnti];
  if (out->measured) {
    out->mean_toa_samples = ul_toa_sum[rnti] / (float)out->measured;
    out->mean_toa_us = out->mean_toa_samples * (1.0e6f / (15000.0f * (float)cd.N));
  }
  return 1;
}

long Engine::getPuschTiming(lsn_pusch_timing_t* out, uint32_t cap) const
{
  const size_t n = std::min<size_t>(cap, ul_last_timing.size());
  if (out && n) std::memcpy(out, ul_last_timing.data(), n * sizeof(lsn_pusch_timing_t));
  return (long)ul_last_timing.size();
}

long Engine::tapUl(int what, uint32_t index, void* out, size_t cap)
{
  if (!ul_set) return LSN_ERROR_INVALID_INPUTS;
  size_t n = 0;
  const void* src = nullptr;
  if (what == 0) { n = (size_t)14 * cd.nre * sizeof(cf32); src = ul_d_grid + (size_t)index * 14 * cd.nre; }  // UL grid of subframe `index`
  else if (what == 1) {  // rate-matched LLRs (UL-SCH order) of grant `index` of the last call
    const LsnUlGrantDev* d = nullptr;
    for (size_t i = 0; i < ul_last_idx.size(); i++)
      if ((uint32_t)ul_last_idx[i] == index) d = &ul_last_gd[i];
    if (!d) return LSN_ERROR_INVALID_INPUTS;
    n = ((size_t)2 * (cell.nslot() - 1) * 12 * d->L_prb - d->q_ri - d->q_cqi) * d->qm * sizeof(int16_t); src = runner_u.d_llr16 + d->llr_off;
  } else if (what == 3 || what == 4) {  // code blocks of grant `index` of the last call in transport-block order: (K, F, E, rv, ok, iters) each / their K + 12 words from k_rm
    const UlTapTb* tb = nullptr;
    for (size_t i = 0; i < ul_last_idx.size() && i < ul_last_tbs.size(); i++)
      if ((uint32_t)ul_last_idx[i] == index) tb = &ul_last_tbs[i];
    if (!tb) return LSN_ERROR_INVALID_INPUTS;
    const UlTapCb* cbs = ul_last_cbs.data() + tb->cb_first;
    for (uint32_t q = 0; q < tb->cb_count; q++) n += what == 3 ? 6 * sizeof(uint32_t) : ((size_t)cbs[q].K + 12) * sizeof(uint32_t);
    if (n > cap) return LSN_ERROR_INVALID_INPUTS;
    uint32_t* o = (uint32_t*)out;
    for (uint32_t q = 0; q < tb->cb_count; q++) {
      const UlTapCb& c = cbs[q];
      if (what == 3) { const uint32_t rec[6] = {c.K, c.F, c.E, c.rv, c.ok, c.iters}; std::memcpy(o, rec, sizeof(rec)); o += 6; continue; }
      if (hipMemcpy(o, runner_u.d_spp + c.spp_off, ((size_t)c.K + 12) * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return LSN_ERROR;
      o += c.K + 12;
    }
    return (long)n;
  } else if (what == 5) {  // private grid rows of grant `index` of the last call (mode 2 of lsn_phy_set_ul_timing)
    if (!ul_last_priv) return LSN_ERROR_INVALID_INPUTS;
    long row = -1;
    for (size_t i = 0; i < ul_last_idx.size(); i++)
      if ((uint32_t)ul_last_idx[i] == index) row = (long)i;
    if (row < 0) return LSN_ERROR_INVALID_INPUTS;
    n = (size_t)cd.nsym * cd.nre * sizeof(cf32); src = ul_d_priv + (size_t)row * 14 * cd.nre;
  } else return LSN_ERROR_INVALID_INPUTS;
  if (n > cap) return LSN_ERROR_INVALID_INPUTS;
  if (hipMemcpy(out, src, n, hipMemcpyDeviceToHost) != hipSuccess) return LSN_ERROR;
  return (long)n;
}

}  // namespace lsn

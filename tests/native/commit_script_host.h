// commit_script_host.h - test glue (NOT product): the product's commit walk (csrc/host/lsn_commit.h) with a host whose PDSCH decoder is a script, shared by
// lsn_hosttest.cc (tests/test_ref_decode.py) and test_commit_walk.cc (the sanitizer program).  Every decode is made on demand, configured by configure_decode
// like Engine::newJob's.
#pragma once
#include "../../ltesniffer_amd/csrc/host/lsn_commit.h"
#include <cstring>
#include <memory>

using namespace lsn;

typedef int (*lsnh_script_fn)(void* user, const uint32_t* call16, float p_a, uint8_t* payload0, uint8_t* payload1, int32_t* crc2);
struct hcommit {
  Cell cell; std::unique_ptr<FalconSearch> s; MCSTracking mcs; HarqDatabase harq; std::unique_ptr<RNTIManager> rm;
  CommitCfg cfg; uint32_t now = 0; lsnh_script_fn script = nullptr; void* script_user = nullptr;
  // one subframe's jobs and records
  std::vector<JobRes> jres; std::vector<PdschGrant> grants; std::vector<uint8_t> payload; std::vector<UeSpecConfig> setups;
  struct Rec { uint32_t kind, tti, rnti, len, off; };
  std::vector<Rec> recs;
};
struct CommitScriptHost {
  hcommit& h; SubframeCtx& c;
  static constexpr size_t TB_STRIDE = 16384;   // (the oracle's payload stride: the largest transport block has 12 237 bytes)
  int attempt(CommitDci& d, int t, float p_a_now)
  {
    if (d.job[t] >= 0) return d.job[t];
    const DlEntry& e = c.dl[d.di];
    PdschGrant g; float p_a;
    if (!configure_decode(h.cell, 0, e, t, p_a_now, c.sfn, g, p_a)) return -1;
    JobRes jr;
    jr.done = 1; jr.p_a = p_a;
    const size_t off = h.payload.size();
    h.payload.resize(off + 2 * TB_STRIDE);
    for (int i = 0; i < 2; i++) { jr.enabled[i] = g.tb[i].enabled ? 1 : 0; jr.len[i] = g.tb[i].tbs / 8; jr.payload_off[i] = (uint32_t)(off + i * TB_STRIDE); }
    if (g.tb[0].enabled || g.tb[1].enabled) {  // the 16 call words of oracle/o_worker.c: decode_grant_harq
      uint32_t call[16] = {c.sfn * 10 + c.sf_idx, e.rnti, g.nof_re, (uint32_t)g.tx_scheme, g.pmi, g.nof_layers};
      for (int i = 0; i < 2; i++) {
        uint32_t* w = call + 6 + 5 * i;
        const GrantTb& tb = g.tb[i];
        w[0] = tb.enabled ? 1u : 0u; w[1] = tb.enabled ? (uint32_t)tb.mod : 0; w[2] = tb.enabled ? (uint32_t)tb.tbs : 0; w[3] = tb.enabled ? (uint32_t)tb.rv : 0; w[4] = tb.enabled ? tb.cw_idx : 0;
      }
      int32_t c2[2] = {0, 0};
      h.script(h.script_user, call, p_a, h.payload.data() + off, h.payload.data() + off + TB_STRIDE, c2);
      for (int i = 0; i < 2; i++) {
        const int tbs = g.tb[i].tbs;
        if (!(g.tb[i].enabled && tbs > 0 && c2[i] != 0)) continue;
        jr.crc[i] = 1;
        if (tbs >= 8 && rnti_name(e.rnti)[0] == 'C') {  // Engine::takeVerdicts: the RRCConnectionSetups of a passed C-RNTI block, parsed ahead of the walk
          UeSpecConfig sc[20];
          const int n = MCSTracking::setups_of_pdu(h.payload.data() + jr.payload_off[i], tbs / 8, sc, 20, true);
          if (n > 0) { jr.setup_first[i] = (uint32_t)h.setups.size(); jr.nsetup[i] = (uint8_t)n; h.setups.insert(h.setups.end(), sc, sc + n); }
        }
      }
    }
    h.jres.push_back(jr); h.grants.push_back(g);
    return d.job[t] = (int)h.jres.size() - 1;
  }
  const JobRes& result(int j) const { return h.jres[j]; }
  int tbs(int j, int tb) const { return h.grants[j].tb[tb].tbs; }
  const uint8_t* payload(uint32_t off) const { return h.payload.data() + off; }
  int mimo_verdict(const CommitDci& d, int t) const
  {
    const DlEntry& e = c.dl[d.di];
    PdschGrant g = t ? e.grant256 : e.grant64;
    return -dl_sniffer_config_mimo(h.cell, e.format, e.dci, g);
  }
  void record(const char* name, uint32_t off, uint32_t len, uint16_t rnti, uint32_t tti, uint8_t)
  {
    h.recs.push_back({name[0] == 'C' ? 1u : name[0] == 'R' ? 2u : name[0] == 'S' ? 3u : 4u, tti, rnti, len, off});
  }
  void rar(const uint8_t* pdu, int len)  // Engine::unpackRar, both threads' halves
  {
    RarEntry r[32];
    const int n = rar_parse(h.cell, pdu, len, r, 32);
    for (int i = 0; i < n; i++) { h.rm->activateAndRefresh(r[i].t_crnti, 0, RM_ACT_RAR); h.mcs.update_rar_time_crnti(r[i].t_crnti, h.now); }
  }
  void learn_setups(const JobRes& jr, int tb, uint16_t rnti, bool any_lcid) { if (jr.nsetup[tb]) h.mcs.learn_setups(h.setups.data() + jr.setup_first[tb], jr.nsetup[tb], rnti, h.now, any_lcid); }
  void learn_pdu(const uint8_t* pdu, int len, uint16_t rnti) { h.mcs.learn_from_pdu(pdu, len, rnti, h.now); }
  // the scripted decoder is a pure function of (tti, RNTI, block, size): the combined decode of a retransmission gets the verdict and bytes of the decode made ahead
  void harq_store(int, int, size_t) {}
  bool harq_combined_decode(int j, int tb, size_t, uint32_t& payload_off) { payload_off = h.jres[j].payload_off[tb]; return h.jres[j].crc[tb] != 0; }
  void harq_size_from_database(CommitDci& d)
  {
    DlEntry& e = c.dl[d.di];
    if (!collection_last_tbs(true, TABLE_64QAM, e, h.harq)) return;
    d.tbs0_64 = e.grant64.tb[0].tbs;
    d.job[0] = -1; e.job[0] = -1;
  }
  void publish(uint16_t) {}
};
inline void commit_script_init(hcommit& h, uint32_t nof_prb, uint32_t nof_ports, uint32_t cell_id, uint32_t cp, int mcs_tracking_mode, int harq_mode, uint32_t nof_rx)
{
  h.cell.nof_prb = nof_prb; h.cell.nof_ports = nof_ports; h.cell.id = cell_id; h.cell.cp = cp;
  h.cfg.mcs_tracking_mode = mcs_tracking_mode; h.cfg.harq_mode = harq_mode != 0; h.cfg.nof_rx = nof_rx;
  h.s.reset(new FalconSearch(5, 0.99, false));
  const uint32_t ncce[3] = {20, 54, 87};
  h.s->setCell(h.cell, ncce);
  h.rm.reset(new RNTIManager(NOF_FORMATS, 304 / 5, 5));
}
// one subframe of n accepted DCI - meta6 = (rnti, format, L, ncce, histval, nof_bits) each, payload bits one byte per bit, 128 per DCI - through
// FalconSearch::finishSubframe, the commit view and the walk; leaves the subframe's records in h.recs, their bytes in h.payload
inline void commit_script_subframe(hcommit& h, uint32_t sfn, uint32_t sf_idx, uint32_t cfi, uint32_t n, const uint32_t* meta6, const uint8_t* bits)
{
  SubframeCtx c;
  c.reset(sfn * 10 + sf_idx);
  c.cfi = cfi; c.searched = true;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* m = meta6 + 6 * i;
    unsigned long long w = 0;
    for (uint32_t b = 0; b < m[5] && b < 64; b++) w |= (unsigned long long)(bits[128 * i + b] & 1) << (63 - b);
    c.raw.push_back(AcceptedDci{(uint16_t)m[0], (uint8_t)m[1], (uint8_t)m[2], (uint16_t)m[3], (uint16_t)m[5], m[4], w});
  }
  h.s->finishSubframe(c);
  std::vector<CommitDci> view;
  commit_view_append(c, view);
  h.jres.clear(); h.grants.clear(); h.payload.clear(); h.setups.clear(); h.recs.clear();
  std::vector<McsTable> tables;
  CommitScriptHost host{h, c};
  commit_walk_subframe(h.cfg, h.mcs, h.harq, c, view.data(), (uint32_t)view.size(), h.now, tables, host);
}

// lsn_commit.h - the downlink commit walk: PDSCH_Decoder::decode_dl_mode (DL_Sniffer_PDSCH.cc:881-1291) over the accepted DCIs of one subframe, HIP-free.
// The walk owns the ORDER of every decision - table of each DCI, gate, known-table decode or 64QAM-then-256QAM trial, HARQ verdict per transport block, what
// becomes a record, what the tracking database learns and counts - and works on the tracking and HARQ databases; everything that is chunk, job or device comes
// from a host object (the engine's adapter in lsn_engine.cc; a scripted decoder in tests/native).  Product code: nothing from oracle/ is included or linked.
#pragma once
#include "lsn_lte.h"
#include "lsn_search.h"
#include "lsn_types.h"
#include <vector>

namespace lsn {

// Compact views for the sequential commit thread (it walks them linearly instead of chasing the wide DlEntry / DecodeJob records that
// other threads wrote): one JobRes per decode job (same index), one CommitDci per accepted downlink DCI in (subframe, acceptance) order.
struct JobRes {
  uint8_t done = 0, crc[2] = {0, 0}, enabled[2] = {0, 0};
  uint8_t nsetup[2] = {0, 0};          // RRCConnectionSetups found in a CRC-ok transport block (pre-parsed by the thread that ran the decode)
  float p_a = 0.0f;
  uint32_t payload_off[2] = {0, 0};
  int32_t len[2] = {0, 0};             // tbs / 8
  uint32_t setup_first[2] = {0, 0};    // into the host's list of pre-parsed setups (Chunk::setup_cfgs)
};
struct CommitDci {
  uint16_t rnti = 0; uint8_t format = 0, flags = 0;   // flags: 1 unpack_ok, 2 ok64, 4 ok256, 8 grant64 has two TBs, 16 grant256 has two TBs
  uint8_t en64 = 0, en256 = 0, mcs_idx[2] = {0, 0};   // en*: bit i = tb[i].enabled of that table's grant
  int32_t tbs0_64 = 0, tbs0_256 = 0;                  // tb[0].tbs of the two grants
  int32_t job[2] = {-1, -1};
  uint32_t di = 0;                                    // index in SubframeCtx::dl (slow path: a decode has to be created at commit)
};
// the CommitDci rows of one finished subframe (FalconSearch::finishSubframe), appended in acceptance order
void commit_view_append(const SubframeCtx& c, std::vector<CommitDci>& out);

// decode_dl_mode's gate (:887-889) on the grant of the table the DCI was collected under (falcon_dci.c:284-310: table_view)
struct CommitGate {
  bool has64, has256, dci_rnti_ok;
  int cur_t;          // the table of the statistics grant: 1 = 256QAM
  bool cur_has;
  int32_t cur_tbs0;   // tb[0].tbs of that grant (0 when it was not computed)
  uint8_t cur_en;     // its enabled bits
  bool two_tb, gate;
};
inline CommitGate commit_gate(const CommitDci& d, McsTable table, uint32_t nof_rx)
{
  const TableView tv = table_view(table, d.rnti, d.flags & 1, d.flags & 2, d.flags & 4);  // falcon_dci.c:284-310
  CommitGate g;
  g.has64 = tv.has64; g.has256 = tv.has256; g.dci_rnti_ok = tv.dci_rnti_ok;
  g.cur_t = table == TABLE_256QAM ? 1 : 0;
  g.cur_has = g.cur_t ? g.has256 : g.has64;
  g.cur_tbs0 = g.cur_has ? (g.cur_t ? d.tbs0_256 : d.tbs0_64) : 0;
  g.cur_en = g.cur_has ? (g.cur_t ? d.en256 : d.en64) : 0;
  g.two_tb = (g.has64 && (d.flags & 8)) || (g.has256 && (d.flags & 16));
  g.gate = (g.cur_tbs0 > 0 && g.dci_rnti_ok && !(nof_rx == 1 && g.two_tb)) || d.rnti == PRNTI;  // :887-889
  return g;
}

// One srsran_ue_dl_decode_pdsch call as the reference configures it: the grant of the table tried, dl_sniffer_config_mimo, the redundancy version of an SI-RNTI
// grant without one (:891-897: on the 64QAM-table grant, the one the gate looked at) or of UL mode (run_decode / run_rar_decode, :240-247,694-701), pdsch_cfg->p_a (DL mode looks the UE's p-a up before every decode,
// :926-927; the UL-mode decoders never set it and run with the -3 dB of SubframeWorker::set_pdsch_uecfg, SubframeWorker.cc:370).
// false: dl_sniffer_config_mimo rejects the grant.
bool configure_decode(const Cell& cell, int sniffer_mode, const DlEntry& e, int table, float p_a, uint32_t sfn, PdschGrant& grant, float& p_a_out);

struct CommitCfg { int mcs_tracking_mode = 0; bool harq_mode = false; uint32_t nof_rx = 1; };

// The walk over one searched subframe: d[0 .. n) are its CommitDci rows, `now` the tracking database's clock, `tables` scratch.  Host (inlined, one flat set):
//   int  attempt(CommitDci& d, int t, float p_a_now)                   the decode of d with table t (0: 64QAM, 1: 256QAM) and this p-a: a job index, -1 without one
//   const JobRes& result(int job); int tbs(int job, int tb); const uint8_t* payload(uint32_t off)
//   int  mimo_verdict(const CommitDci& d, int t)                        dl_sniffer_config_mimo's 0 / -1 / -2 / -3 for a DCI that got no job
//   void record(const char* name, uint32_t off, uint32_t len, uint16_t rnti, uint32_t tti, uint8_t tb)
//   void rar(const uint8_t* pdu, int len)
//   void learn_setups(const JobRes& jr, int tb, uint16_t rnti, bool any_lcid); void learn_pdu(const uint8_t* pdu, int len, uint16_t rnti)
//   void harq_store(int job, int tb, size_t slot); bool harq_combined_decode(int job, int tb, size_t slot, uint32_t& payload_off)
//   void harq_size_from_database(CommitDci& d)                          collection_last_tbs on the wide entry; d.tbs0_64 and d.job[0] follow
//   void publish(uint16_t rnti)
template <class Host>
void commit_walk_subframe(const CommitCfg& cfg, MCSTracking& mcs_tracking, HarqDatabase& harq_db, const SubframeCtx& c, CommitDci* dcis, uint32_t n, uint32_t now,
                          std::vector<McsTable>& tables, Host& host)
{
  // DCICollection.cc:107-134: the table of every DCI of this subframe is fixed before any of them is decoded
  tables.resize(n);
  for (uint32_t k = 0; k < n; k++) tables[k] = collection_table(cfg.mcs_tracking_mode, dcis[k].rnti, (DciFormat)dcis[k].format, mcs_tracking, now);
  // addCandidate looks the table up for EVERY accepted DCI, format 0 included: an uplink grant refreshes the entry's time stamp too
  if (cfg.mcs_tracking_mode == 1)
    for (const UlEntry& u : c.ul)
      if (!(u.rnti == SIRNTI || u.rnti == PRNTI || rnti_israr(u.rnti))) (void)mcs_tracking.find_tracking_info_RNTI_dl(u.rnti, now);
  for (uint32_t k = 0; k < n; k++) {
    CommitDci& d = dcis[k];
    const McsTable table = tables[k];
    // DCICollection.cc:236-251: a reserved MCS index of a 64QAM-table grant takes its size from the HARQ database (harq_mode only).  The plan knew no size for
    // it (0): whatever it decoded for this entry is dropped and the grant is decoded on demand with the size in
    if (cfg.harq_mode && table == TABLE_64QAM && (d.flags & 1)) host.harq_size_from_database(d);
    const CommitGate g = commit_gate(d, table, cfg.nof_rx);
    if (!g.gate) continue;
    const char* name = rnti_name(d.rnti);
    // :926-927: the p-a in force when this DCI is decoded.  A job planned (or speculated) with another value - a connection setup
    // was committed in between - is dropped and decoded again, so results do not depend on how far ahead the pipeline planned
    const float p_a_now = mcs_tracking.get_ue_config_rnti(d.rnti).p_a;
    auto run = [&](int t) -> int { return (t ? g.has256 : g.has64) ? host.attempt(d, t, p_a_now) : -1; };
    // dl_sniffer_config_mimo's verdict for the statistics: a job exists exactly when it was 0, so the function itself only runs again for the rare rejected grant
    auto mimo_of = [&](int t, int job) { return job >= 0 ? 0 : host.mimo_verdict(d, t); };
    bool crc[2] = {false, false};   // pdsch_res[].crc as the statistics see it at the end of the iteration
    int mimo_ret = 0;
    if (table == TABLE_64QAM || table == TABLE_256QAM) {  // :932-1083
      const int j = run(g.cur_t);
      mimo_ret = g.cur_has ? mimo_of(g.cur_t, j) : -1;
      if (j >= 0) {
        const JobRes jr = host.result(j);  // (by value: a combined decode below may append to the host's vectors)
        for (int tb = 0; tb < 2; tb++) {
          crc[tb] = jr.crc[tb] != 0;
          uint32_t poff = jr.payload_off[tb];
          bool combined = false;
          if (cfg.harq_mode && name[0] == 'C' && jr.enabled[tb]) {  // :943-1020: new transmission / retransmission / already decoded, per transport block
            const DlEntry& e = c.dl[d.di];
            const int tbs = host.tbs(j, tb);
            int ent = -1;
            const HarqRet hr = harq_db.is_retransmission(d.rnti, e.dci.pid, tb, e.dci.tb[tb].ndi != 0, tbs, c.sfn, c.sf_idx, ent);
            const size_t slot = ent < 0 ? 0 : ((size_t)ent * HarqDatabase::NPID + (e.dci.pid & 7u)) * 2 + (size_t)tb;
            if (hr == HARQ_NEW_TX) {
              if (!crc[tb]) host.harq_store(j, tb, slot);   // srsran_softbuffer_rx_reset_tbs + this transmission (the buffer is only read again if the block failed)
            } else if (hr == HARQ_RE_TX) {
              crc[tb] = host.harq_combined_decode(j, tb, slot, poff);
              combined = true;
            } else if (hr == HARQ_DECODED) {
              crc[tb] = false;                 // decoded 8 subframes ago: not decoded again, nothing written
            }
            if (hr == HARQ_NEW_TX || hr == HARQ_RE_TX) harq_db.update(ent, e.dci.pid, tb, c.sfn, c.sf_idx, crc[tb], e.dci.tb[tb].ndi != 0, e.dci.tb[tb].rv, tbs, now);
          }
          if (crc[tb] && jr.len[tb] > 0) {
            host.record(name, poff, (uint32_t)jr.len[tb], d.rnti, c.tti, (uint8_t)tb);
            if (name[0] == 'R') host.rar(host.payload(poff), jr.len[tb]);
            if (name[0] == 'C') {
              if (combined) host.learn_pdu(host.payload(poff), jr.len[tb], d.rnti);  // (not pre-parsed: the block was decoded in this turn)
              else host.learn_setups(jr, tb, d.rnti, false);                         // :1041-1070: the SDUs on logical channel 0
            }
          }
        }
      }
    } else {  // unknown table: 64QAM table first, the 256QAM table only if both TBs failed, :1089-1243
      const int j = run(0);
      mimo_ret = g.has64 ? mimo_of(0, j) : -1;
      if (j >= 0) {
        const JobRes& jr = host.result(j);
        for (int tb = 0; tb < 2; tb++) {
          crc[tb] = jr.crc[tb] != 0;
          if (crc[tb] && jr.len[tb] > 0) {
            host.record(name, jr.payload_off[tb], (uint32_t)jr.len[tb], d.rnti, c.tti, (uint8_t)tb);
            if (name[0] == 'R') host.rar(host.payload(jr.payload_off[tb]), jr.len[tb]);
            if (name[0] == 'C') host.learn_setups(jr, tb, d.rnti, true);  // :1133-1160: every SDU, whatever its logical channel
            if (d.mcs_idx[tb] > 0 && d.mcs_idx[tb] < 29 && d.format > FORMAT1A) mcs_tracking.update_RNTI_dl(d.rnti, TABLE_64QAM, now);
          }
        }
      }
      if (!crc[0] && !crc[1] && mimo_ret == 0) {
        const int j2 = run(1);
        mimo_ret = g.has256 ? mimo_of(1, j2) : -1;
        if (j2 >= 0) {
          const JobRes& jr = host.result(j2);
          for (int tb = 0; tb < 2; tb++) {
            if (jr.enabled[tb]) crc[tb] = jr.crc[tb] != 0;
            if (jr.crc[tb] && jr.len[tb] > 0) {
              host.record(name, jr.payload_off[tb], (uint32_t)jr.len[tb], d.rnti, c.tti, (uint8_t)tb);
              if (d.mcs_idx[tb] > 0 && d.mcs_idx[tb] < 28 && d.format > FORMAT1A) mcs_tracking.update_RNTI_dl(d.rnti, TABLE_256QAM, now);
            }
          }
        }
      }
    }
    if (name[0] == 'C' && cfg.mcs_tracking_mode) {  // :1268-1285
      const bool tb_en[2] = {(g.cur_en & 1) != 0, (g.cur_en & 2) != 0};
      mcs_tracking.update_statistic_dl(d.rnti, (DciFormat)d.format, table, tb_en, crc, mimo_ret, now);
    }
    host.publish(d.rnti);
  }
}

}  // namespace lsn

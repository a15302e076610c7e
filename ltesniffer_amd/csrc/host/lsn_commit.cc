// lsn_commit.cc - the parts of the downlink commit walk that are no templates (see lsn_commit.h).  HIP-free product code.
#include "lsn_commit.h"
#include <cmath>

namespace lsn {

void commit_view_append(const SubframeCtx& c, std::vector<CommitDci>& out)
{
  for (size_t di = 0; di < c.dl.size(); di++) {
    const DlEntry& e = c.dl[di];
    CommitDci d;
    d.rnti = e.rnti; d.format = (uint8_t)e.format; d.di = (uint32_t)di;
    d.flags = (uint8_t)((e.unpack_ok ? 1 : 0) | (e.ok64 ? 2 : 0) | (e.ok256 ? 4 : 0) | (e.grant64.nof_tb == 2 ? 8 : 0) | (e.grant256.nof_tb == 2 ? 16 : 0));
    for (int i = 0; i < 2; i++) {
      if (e.grant64.tb[i].enabled) d.en64 |= (uint8_t)(1u << i);
      if (e.grant256.tb[i].enabled) d.en256 |= (uint8_t)(1u << i);
      d.mcs_idx[i] = (uint8_t)e.dci.tb[i].mcs_idx;
      d.job[i] = e.job[i];
    }
    d.tbs0_64 = e.grant64.tb[0].tbs; d.tbs0_256 = e.grant256.tb[0].tbs;
    out.push_back(d);
  }
}

bool configure_decode(const Cell& cell, int sniffer_mode, const DlEntry& e, int table, float p_a, uint32_t sfn, PdschGrant& grant, float& p_a_out)
{
  p_a_out = sniffer_mode == 1 ? -3.0f : p_a;
  grant = table ? e.grant256 : e.grant64;
  if (dl_sniffer_config_mimo(cell, e.format, e.dci, grant) != 0) return false;
  if (sniffer_mode == 1) {  // run_decode / run_rar_decode, DL_Sniffer_PDSCH.cc:240-247,694-701
    for (auto& tb : grant.tb)
      if (tb.enabled && tb.rv < 0) tb.rv = (int)((uint32_t)ceilf(1.5f * (float)((sfn / 2) % 4)) % 4u);
  } else if (table == 0 && e.dci.tb[0].rv < 0 && e.rnti == SIRNTI) {
    // DL_Sniffer_PDSCH.cc:891-897 resolves the missing redundancy version of a format 1C grant on the grant the gate looked at - for the SI-RNTI always the
    // 64QAM-table one.  The 256QAM-table attempt of the unknown-table branch (mcs_tracking_mode 2) is handed on as the DCI left it; both tables give a format 1C
    // grant the same decode, so the engine serves that attempt with the 64QAM-table job (same_decode, lsn_engine.cc) and never sends it to the device (newJob)
    grant.tb[0].rv = 0;
  }
  return true;
}

}  // namespace lsn

// lsn_harq.cc - HARQ soft combining (harq_mode = 1, DL mode): the soft buffers of the HARQ processes, filled and combined by the commit stage
// (see lsn_engine.h: HarqKeep, HarqReq).  Product code: no CPU fallback, nothing from oracle/ is included or linked.
#include "lsn_engine.h"
#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace lsn {

// Block q of the buffer of a (RNTI entity, process, transport block) has its home in the pool at slot * HARQ_SLOT_WORDS + q * HARQ_CB_WORDS.  Inside a commit
// turn the content may lie elsewhere (HarqKeep::loc): a failed new transmission stays in the chunk's keep store, a combination in the turn's scratch area;
// harqFlush brings everything home before the chunk (and with it the keep store) is recycled.  Round 6: retransmissions are combined and decoded in batches
// ahead of the walk (lsn_engine.h: HarqReq) - rounds 4-5 paid one GPU round trip per retransmission inside the sequential turn.
uint64_t Engine::harqMix(uint64_t a, uint64_t b, uint64_t c, uint64_t d)
{
  auto sm = [](uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); };
  return sm(sm(sm(sm(a) ^ b) ^ c) ^ d);
}

// The request a retransmission (job, block) makes when it meets a buffer in the state (ncb_have, ver, ok, loc) - the SAME function serves the walk and the
// scout, so that equal states give equal keys.  A buffer without a first transmission on record for this geometry (ncb_have != n) is taken as it lies in
// the pool, nothing passed (rounds 4-5: hk = HarqKeep{}); the pool does not change inside a turn, so (slot, n) names that content.  false: every block has
// passed already, nothing to combine or decode.
bool Engine::harqRequest(int job, int tb, size_t slot, uint32_t n, uint32_t ncb_have, uint64_t ver, const uint8_t* ok, const uint32_t* loc, HarqReq& q) const
{
  q = HarqReq{};
  q.job = job; q.tb = tb; q.slot = slot; q.n = n;
  uint64_t okmask = 0;
  if (ncb_have != n) {
    q.ver = harqMix(0x52455345u /* reset */, slot, n, 0);
    for (uint32_t i = 0; i < n; i++) { q.ok[i] = 0; q.loc[i] = HARQ_LOC_POOL | (uint32_t)(slot * HARQ_SLOT_WORDS + i * HARQ_CB_WORDS); }
  } else {
    q.ver = ver;
    for (uint32_t i = 0; i < n; i++) { q.ok[i] = ok[i] ? 1 : 0; q.loc[i] = loc[i]; okmask |= (uint64_t)(ok[i] ? 1 : 0) << i; }
  }
  q.key = harqMix(q.ver, ((uint64_t)(uint32_t)job << 1) | (uint64_t)(tb & 1), okmask, n);
  return okmask != ((1ull << n) - 1ull);
}

// The soft data of a decode launch stays with the chunk until its commit (the buffers are filled / combined there): copied behind the decoders of the launch,
// the descriptors of its blocks kept with their place in the chunk's keep store
void Engine::harqKeepSoftData(Chunk& ch, JobRunner& r, const DecodeLaunch& L)
{
  const size_t spp_n = L.place.spp_n;
  if (ch.keep_n + spp_n >= ((size_t)1 << 30)) throw std::runtime_error("harq_mode: the soft data of one chunk exceeds 4 GB (2^30 words) - process smaller batches");   // (HarqKeep::loc: 30-bit word offsets)
  if (ch.keep_n + spp_n > ch.keep_cap) {
    const size_t cap = (ch.keep_n + spp_n) * 2 + (1u << 20);
    uint32_t* nb = nullptr;
    HIP_CHECK(hipMalloc((void**)&nb, cap * sizeof(uint32_t)));
    if (ch.keep_n) HIP_CHECK(hipMemcpy(nb, ch.d_keep, ch.keep_n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    if (ch.d_keep) HIP_CHECK(hipFree(ch.d_keep));
    ch.d_keep = nb; ch.keep_cap = cap;
  }
  HIP_CHECK(hipMemcpyAsync(ch.d_keep + ch.keep_n, r.d_spp, spp_n * sizeof(uint32_t), hipMemcpyDeviceToDevice, r.stream));
  for (auto& tr : L.tbrefs) {
    DecodeJob& j = ch.jobs[tr.job];
    j.keep_first[tr.tb] = (uint32_t)ch.keep_cbs.size(); j.keep_count[tr.tb] = tr.cb_count;
    for (uint32_t q = 0; q < tr.cb_count; q++) {
      LsnCbDev cb = r.h_cbs[tr.cb_first + q];
      cb.spp_off = (uint32_t)(ch.keep_n + L.place.spp_of[tr.cb_first + q]);
      ch.keep_cbs.push_back(cb);
    }
  }
  ch.keep_n += spp_n;
}

// per-block verdicts of this transmission, next to the kept soft data (harqStore / harqCombinedDecode)
void Engine::harqKeepResults(Chunk& ch, JobRunner& r, const DecodeLaunch::TbRef& t)
{
  const DecodeJob& j = ch.jobs[t.job];
  if (ch.keep_res.size() < ch.keep_cbs.size()) ch.keep_res.resize(ch.keep_cbs.size());
  for (uint32_t q = 0; q < t.cb_count && j.keep_count[t.tb] == t.cb_count; q++) ch.keep_res[j.keep_first[t.tb] + q] = r.h_cbres_pinned[t.cb_first + q];
}

void Engine::harqStore(Chunk& ch, int job, int tb, size_t slot)
{
  const DecodeJob& j = ch.jobs[job];
  const uint32_t n = j.keep_count[tb];
  if (!n || n > HARQ_MAX_CB) { harq_keep.erase(slot); return; }   // nothing stored for this transmission: what the slot held belongs to an older one and must not be combined with
  // cb_crc / data of the soft buffer: what passed in this (failed) transmission is remembered, a retransmission decodes the other blocks only
  HarqKeep& hk = harq_keep[slot];
  hk.ncb = n;
  hk.ver = harqMix(0x53544F52u /* store */, ch.gseq, (uint64_t)(uint32_t)job, (uint64_t)tb);
  uint32_t boff = 0;
  for (uint32_t q = 0; q < n; q++) {
    const LsnCbDev& cb = ch.keep_cbs[j.keep_first[tb] + q];
    const LsnCbRes cr = j.keep_first[tb] + q < ch.keep_res.size() ? ch.keep_res[j.keep_first[tb] + q] : LsnCbRes{};
    hk.ok[q] = cr.ok ? 1 : 0; hk.rem_a[q] = cr.rem_a; hk.K[q] = cb.K;
    const uint8_t* pb = ch.h_payload.data() + j.payload_off[tb] + boff;
    hk.bytes[q].assign(pb, pb + cb.out_bytes);
    boff += cb.out_bytes;
    hk.loc[q] = HARQ_LOC_KEEP | cb.spp_off;   // this transmission, where it lies in the chunk's keep store: nothing reads it before a retransmission combines with it
  }
  harq_touched.push_back(slot);
}

// end of the commit turn: the blocks that do not lie at home go there in at most one launch (rounds 4 / early 5 paid an upload, a launch and a stream
// synchronisation per failed transport block: 2.7 k subframes/s on the gated HARQ leg)
void Engine::harqFlush(Chunk& ch, JobRunner& r)
{
  ScopeTimer timer(r.perf.ms_harq[2]);
  std::vector<LsnCbDev> cp;
  std::sort(harq_touched.begin(), harq_touched.end());
  harq_touched.erase(std::unique(harq_touched.begin(), harq_touched.end()), harq_touched.end());
  for (size_t slot : harq_touched) {
    auto it = harq_keep.find(slot);
    if (it == harq_keep.end()) continue;
    HarqKeep& hk = it->second;
    for (uint32_t q = 0; q < hk.ncb && q < HARQ_MAX_CB; q++) {
      const uint32_t home = HARQ_LOC_POOL | (uint32_t)(slot * HARQ_SLOT_WORDS + q * HARQ_CB_WORDS);
      if (hk.loc[q] == home) continue;
      LsnCbDev cb{};
      cb.K = hk.K[q]; cb.reserved = hk.loc[q]; cb.spp_off = home;
      cp.push_back(cb);
      hk.loc[q] = home;
    }
  }
  harq_touched.clear();
  for (auto& kv : harq_cache) if (!kv.second.used) r.perf.nof_harq_combines[3]++;
  harq_cache.clear();
  harq_scratch_n = 0;
  if (cp.empty()) return;
  const uint32_t n = (uint32_t)cp.size();
  grow_host(harq_h_store, harq_h_store_cap, n, r.stream);
  grow_dev(harq_d_store, harq_d_store_cap, n, r.stream);
  std::memcpy(harq_h_store, cp.data(), n * sizeof(LsnCbDev));
  lsn_launch_upload(harq_d_store, harq_h_store, n * sizeof(LsnCbDev), r.stream);
  lsn_launch_harq_combine(harq_d_store, n, ch.d_keep, d_harq_pool, d_harq_scratch, true, r.stream);
  HIP_CHECK(hipStreamSynchronize(r.stream));   // the chunk's keep store is recycled with the chunk
}

// combine + decode a batch of requests: one descriptor upload, one combination launch, one decoder launch per wavefront class, one download, one wait
void Engine::harqRunBatch(Chunk& ch, JobRunner& r, const std::vector<HarqReq>& reqs)
{
  if (reqs.empty()) return;
  ScopeTimer timer(r.perf.ms_harq[1]);
  hipStream_t st = r.stream;
  struct Ref { uint32_t req, q, out; };
  std::vector<LsnCbDev> cbs;
  std::vector<Ref> refs;
  uint32_t out = 0;
  size_t words = harq_scratch_n;
  for (uint32_t i = 0; i < reqs.size(); i++) {
    const HarqReq& q = reqs[i];
    const DecodeJob& j = ch.jobs[q.job];
    for (uint32_t b = 0; b < q.n; b++) {
      if (q.ok[b]) continue;   // srsRAN: if (!softbuffer->cb_crc[cb_idx]) { rate de-matching into the buffer, decoding } - a passed block is left alone
      LsnCbDev cb = ch.keep_cbs[j.keep_first[q.tb] + b];
      cb.e_off = cb.spp_off;                       // this transmission, in the chunk's keep store
      cb.reserved = q.loc[b];                      // what the buffer holds, wherever it lies
      cb.spp_off = (uint32_t)words; words += LSN_SPP_WORDS(cb.K);
      cb.res_idx = (uint32_t)cbs.size(); cb.dep = LSN_CB_NODEP; cb.out_off = out;
      refs.push_back({i, b, out});
      out += cb.out_bytes;
      cbs.push_back(cb);
    }
  }
  const uint32_t nd = (uint32_t)cbs.size();
  if (!nd) return;
  if (words > harq_scratch_cap || words >= (1u << 30)) throw std::runtime_error("HARQ scratch area exhausted");   // (sized by the caller: harqEnsureScratch)
  harq_scratch_n = words;
  grow_host(r.h_cbs_pinned, r.h_cbs_cap, nd, st);
  grow_dev(r.d_cbs, r.cbs_cap, nd, st);
  if (nd > r.cbres_cap) grow_dev(r.d_cbres, r.cbres_cap, nd, st);
  grow_host(r.h_cbres_pinned, r.h_cbres_cap, nd, st);
  grow_dev(r.d_payload, r.payload_cap, (size_t)out + 16, st);
  grow_host(r.h_payload_pinned, r.h_payload_cap, (size_t)out + 16, st);
  // launch order: two-wavefront class first, each class by descending size (the longest first); results stay addressable through res_idx
  const TurboOrder to = turbo_classic_order(cbs);
  for (uint32_t i = 0; i < nd; i++) r.h_cbs_pinned[i] = cbs[to.order[i]];
  lsn_launch_upload(r.d_cbs, r.h_cbs_pinned, nd * sizeof(LsnCbDev), st);
  lsn_launch_harq_combine(r.d_cbs, nd, ch.d_keep, d_harq_pool, d_harq_scratch, false, st);
  lsn_launch_turbo(cd, r.d_cbs, d_harq_scratch, r.d_payload, r.d_cbres, to.n128, to.kmax128, nd - to.n128, to.kmax64, st);
  {
    LsnCopySegs dn;   // verdicts + payload bytes down in one launch
    dn.add(r.h_cbres_pinned, r.d_cbres, nd * sizeof(LsnCbRes));
    dn.add(r.h_payload_pinned, r.d_payload, out);
    lsn_launch_copy_multi(dn, true, st);
  }
  HIP_CHECK(hipEventRecord(r.ev_done, st));
  waitEvent(r.ev_done, 3000);   // inside the sequential commit turn: short naps (the decode threads' waits are milliseconds long and nap 50 us)
  r.perf.nof_harq_combines[0]++;
  for (uint32_t i = 0; i < reqs.size(); i++) { HarqDone& d = harq_cache[reqs[i].key]; d = HarqDone{}; d.req = reqs[i]; }
  for (uint32_t k = 0; k < nd; k++) {
    const Ref& f = refs[k];
    HarqDone& d = harq_cache[reqs[f.req].key];
    const LsnCbRes& cr = r.h_cbres_pinned[k];   // (res_idx = k: the index before sorting)
    d.ok[f.q] = cr.ok ? 1 : 0; d.rem_a[f.q] = cr.rem_a; d.iters[f.q] = cr.iters;
    d.loc[f.q] = HARQ_LOC_SCRATCH | cbs[k].spp_off;
    d.bytes[f.q].assign(r.h_payload_pinned + f.out, r.h_payload_pinned + f.out + cbs[k].out_bytes);
  }
}

// The combined decodes the walk over this chunk will probably ask for, as far as their inputs are known now: the walk's HARQ decisions (commitChunk,
// known-table branch) replayed on COPIES of the process database and of the touched buffers' states, with the tables, jobs and p-a values as they stand at
// the start of the turn.  A retransmission whose result is in harq_cache continues its buffer's chain; one without becomes a request, and the chain of that
// buffer stops for this pass (its later retransmissions need the result first).  Nothing but speed depends on how well this guesses: the walk makes its own
// requests and takes a result only under the key of exactly its inputs.
void Engine::harqScout(Chunk& ch, std::vector<HarqReq>& out, bool first_pass)
{
  out.clear();
  struct View { uint32_t ncb = 0; uint8_t ok[16] = {}; uint32_t rem_a[16] = {}, loc[16] = {}; uint64_t ver = 0; bool pending = false; };
  std::unordered_map<size_t, View> ov;
  auto view = [&](size_t slot) -> View& {
    auto it = ov.find(slot);
    if (it != ov.end()) return it->second;
    View v;
    auto k = harq_keep.find(slot);
    if (k != harq_keep.end()) {
      v.ncb = k->second.ncb; v.ver = k->second.ver;
      for (int q = 0; q < 16; q++) { v.ok[q] = k->second.ok[q]; v.rem_a[q] = k->second.rem_a[q]; v.loc[q] = k->second.loc[q]; }
    }
    return ov.emplace(slot, v).first->second;
  };
  // The transport blocks the walk will put to the process database, in walk order (tables, jobs and p-a values as they stand at the start of the turn: the
  // same in every pass of this turn, so the list is made by the first pass and replayed by the others).  job < 0: the database's 10 s timer.
  if (first_pass) {
    harq_events.clear();
    uint32_t cnt = commit_sf_cnt;
    for (uint32_t sf = 0; sf < ch.nsf; sf++, cnt++) {
      const SubframeCtx& c = ch.ctx[sf];
      if (cnt && (cnt % 10000u) == 0) { HarqEvent ev; ev.job = -1; ev.now = cnt; harq_events.push_back(ev); }
      if (!c.searched) continue;
      for (uint32_t k = ch.cdci_first[sf]; k < ch.cdci_first[sf + 1]; k++) {
        const CommitDci& d = ch.cdci[k];
        const char* name = rnti_name(d.rnti);
        if (name[0] != 'C') continue;
        const McsTable table = collection_table_from(cfg.mcs_tracking_mode, d.rnti, (DciFormat)d.format, [&] { return mcs_tracking.peek(d.rnti); });
        if (!(table == TABLE_64QAM || table == TABLE_256QAM)) continue;
        const DlEntry& e = c.dl[d.di];
        if (table == TABLE_64QAM && e.unpack_ok && ((e.grant64.tb[0].enabled && e.grant64.tb[0].mcs_idx > 28) || (e.grant64.tb[1].enabled && e.grant64.tb[1].mcs_idx > 28)))
          continue;   // (a reserved MCS index takes its size from the database at commit and is decoded there)
        const CommitGate g = commit_gate(d, table, dlRx());   // (C-RNTIs only here: the gate's paging clause does not apply)
        if (!g.gate) continue;
        const int j = d.job[g.cur_t];
        if (!g.cur_has || j < 0 || !ch.jres[j].done || ch.jres[j].p_a != mcs_tracking.get_ue_config_rnti(d.rnti).p_a) continue;
        const JobRes& jr = ch.jres[j];
        for (int tb = 0; tb < 2; tb++) {
          if (!jr.enabled[tb]) continue;
          HarqEvent ev;
          ev.job = j; ev.now = cnt; ev.sfn = c.sfn; ev.sf_idx = c.sf_idx; ev.rnti = d.rnti; ev.pid = (uint8_t)e.dci.pid; ev.tb = (uint8_t)tb;
          ev.ndi = e.dci.tb[tb].ndi != 0; ev.rv = (uint8_t)e.dci.tb[tb].rv; ev.tbs = ch.jobs[j].grant.tb[tb].tbs; ev.crc = jr.crc[tb] != 0; ev.n = ch.jobs[j].keep_count[tb];
          harq_events.push_back(ev);
        }
      }
    }
  }
  HarqDatabase db = harq_db;
  for (const HarqEvent& ev : harq_events) {
    if (ev.job < 0) { db.update_database(ev.now); continue; }
    const int j = ev.job, tb = ev.tb;
    int ent = -1;
    const HarqRet hr = db.is_retransmission(ev.rnti, ev.pid, tb, ev.ndi, ev.tbs, ev.sfn, ev.sf_idx, ent);
    const size_t slot = ent < 0 ? 0 : ((size_t)ent * HarqDatabase::NPID + (ev.pid & 7u)) * 2 + (size_t)tb;
    bool crc = ev.crc;
    const uint32_t n = ev.n;
    if (hr == HARQ_NEW_TX) {
      if (!crc) {
        View& v = view(slot);
        v = View{};
        if (n && n <= HARQ_MAX_CB) {
          v.ncb = n; v.ver = harqMix(0x53544F52u, ch.gseq, (uint64_t)(uint32_t)j, (uint64_t)tb);
          for (uint32_t q = 0; q < n; q++) {
            const size_t ki = ch.jobs[j].keep_first[tb] + q;
            const LsnCbRes cr = ki < ch.keep_res.size() ? ch.keep_res[ki] : LsnCbRes{};
            v.ok[q] = cr.ok ? 1 : 0; v.rem_a[q] = cr.rem_a; v.loc[q] = HARQ_LOC_KEEP | ch.keep_cbs[ki].spp_off;
          }
        }
      }
    } else if (hr == HARQ_RE_TX) {
      crc = false;
      if (n && n <= HARQ_MAX_CB) {
        View& v = view(slot);
        if (!v.pending) {
          HarqReq q;
          const bool work = harqRequest(j, tb, slot, n, v.ncb, v.ver, v.ok, v.loc, q);
          if (v.ncb != n) { v = View{}; v.ncb = n; v.ver = q.ver; for (uint32_t b = 0; b < n; b++) v.loc[b] = q.loc[b]; }
          bool have = true;
          if (work) {
            auto it = harq_cache.find(q.key);
            if (it == harq_cache.end()) { out.push_back(q); v.pending = true; have = false; }
            else {
              const HarqDone& dn = it->second;
              for (uint32_t b = 0; b < n; b++)
                if (!v.ok[b]) { v.rem_a[b] = dn.rem_a[b]; v.loc[b] = dn.loc[b]; v.ok[b] = dn.ok[b]; }
              v.ver = q.key;
            }
          }
          if (have) {  // the verdict as far as the scout can tell (every block passed, CRC24A over the blocks; the parity-word and length tests are the walk's)
            TbVerdict tv;
            for (int b = (int)n - 1; b >= 0; b--) tv.add(v.ok[b] != 0, v.rem_a[b], ch.keep_cbs[ch.jobs[j].keep_first[tb] + b].out_bytes);
            crc = tv.all_ok && tv.rem == 0;
          }
        }
      }
    } else if (hr == HARQ_DECODED) {
      crc = false;
    }
    if (hr == HARQ_NEW_TX || hr == HARQ_RE_TX) db.update(ent, ev.pid, tb, ev.sfn, ev.sf_idx, crc, ev.ndi, ev.rv, ev.tbs, ev.now);
  }
}

// The retransmissions of this chunk, combined and decoded in a few batches ahead of the walk (harqScout): pass p serves the p-th retransmission in a row of the
// same buffer.  The scratch area is empty here (harqFlush of the previous turn): it may be given a new size
void Engine::harqBatchAhead(Chunk& ch, JobRunner& r)
{
  harq_scratch_n = 0;
  const size_t want = std::min<size_t>(ch.keep_n + 4096, (size_t)(1u << 30) - 1);
  if (want > harq_scratch_cap) grow_dev(d_harq_scratch, harq_scratch_cap, want, r.stream);
  std::vector<HarqReq> reqs;
  for (int pass = 0; pass < 8; pass++) {
    const double t0 = now_ms();
    harqScout(ch, reqs, pass == 0);
    r.perf.ms_harq[0] += now_ms() - t0;
    if (reqs.empty()) break;
    size_t need = 0;
    for (const HarqReq& q : reqs)
      for (uint32_t b = 0; b < q.n; b++)
        if (!q.ok[b]) need += LSN_SPP_WORDS(ch.keep_cbs[ch.jobs[q.job].keep_first[q.tb] + b].K);
    if (harq_scratch_n + need > harq_scratch_cap) break;   // (what does not fit is decoded by the walk itself)
    harqRunBatch(ch, r, reqs);
  }
}

bool Engine::harqCombinedDecode(Chunk& ch, JobRunner& r, int job, int tb, size_t slot, uint32_t& payload_off)
{
  const DecodeJob& j = ch.jobs[job];
  const uint32_t n = j.keep_count[tb];
  if (!n || n > HARQ_MAX_CB) return false;
  HarqKeep& hk = harq_keep[slot];
  HarqReq q;
  const bool work = harqRequest(job, tb, slot, n, hk.ncb, hk.ver, hk.ok, hk.loc, q);
  if (hk.ncb != n) {  // (no first transmission on record for this geometry: nothing passed before)
    hk = HarqKeep{};
    hk.ncb = n; hk.ver = q.ver;
    for (uint32_t b = 0; b < n; b++) hk.loc[b] = q.loc[b];
  }
  for (uint32_t b = 0; b < n; b++) hk.K[b] = ch.keep_cbs[j.keep_first[tb] + b].K;
  const HarqDone* dn = nullptr;
  if (work) {
    auto it = harq_cache.find(q.key);
    if (it != harq_cache.end() && !(it->second.req.ver == q.ver && it->second.req.job == job && it->second.req.tb == tb && it->second.req.n == n && std::memcmp(it->second.req.ok, q.ok, 16) == 0)) it = harq_cache.end();  // (a hash collision)
    if (it == harq_cache.end()) {
      // not foreseen by the scout: decoded now, alone (a round trip inside the turn, as every retransmission was in rounds 4-5)
      size_t need = 0;
      for (uint32_t b = 0; b < n; b++) if (!q.ok[b]) need += LSN_SPP_WORDS(hk.K[b]);
      if (harq_scratch_n + need > harq_scratch_cap) {  // scratch area full: everything goes home first (the unused results of the batches are lost with it)
        harqFlush(ch, r);
        harqRequest(job, tb, slot, n, hk.ncb, hk.ver, hk.ok, hk.loc, q);
        if (need > harq_scratch_cap) { HIP_CHECK(hipStreamSynchronize(r.stream)); grow_dev(d_harq_scratch, harq_scratch_cap, need, r.stream); }
      }
      std::vector<HarqReq> one{q};
      harqRunBatch(ch, r, one);
      r.perf.nof_harq_combines[2]++;
      r.perf.nof_ondemand_decodes++;
      it = harq_cache.find(q.key);
    } else {
      r.perf.nof_harq_combines[1]++;
    }
    it->second.used = true;
    dn = &it->second;
    for (uint32_t b = 0; b < n; b++) {
      if (hk.ok[b]) continue;
      r.perf.nof_turbo_iterations += dn->iters[b];
      hk.rem_a[b] = dn->rem_a[b];
      hk.bytes[b] = dn->bytes[b];
      hk.loc[b] = dn->loc[b];
      // (ok is set below, after the verdict of THIS pass has been taken)
    }
    hk.ver = q.key;
    harq_touched.push_back(slot);
  }
  // transport-block verdict, as in runJobs: every block passed (now or in an earlier transmission), CRC24A over the assembled blocks
  TbVerdict v;
  uint32_t total = 0;
  for (int b = (int)n - 1; b >= 0; b--) v.add(hk.ok[b] || (dn && dn->ok[b] != 0), hk.rem_a[b], ch.keep_cbs[j.keep_first[tb] + b].out_bytes);
  for (uint32_t b = 0; b < n; b++) total += (uint32_t)hk.bytes[b].size();
  const int tbs = j.grant.tb[tb].tbs;
  payload_off = (uint32_t)ch.h_payload.size();
  ch.h_payload.resize(ch.h_payload.size() + (((size_t)total + 15) & ~(size_t)15));
  {
    uint8_t* dst = ch.h_payload.data() + payload_off;
    for (uint32_t b = 0; b < n; b++) { std::memcpy(dst, hk.bytes[b].data(), hk.bytes[b].size()); dst += hk.bytes[b].size(); }
  }
  for (uint32_t b = 0; b < n; b++)
    if (!hk.ok[b] && dn && dn->ok[b]) hk.ok[b] = 1;
  if ((uint64_t)total * 8ull < (uint64_t)tbs + 24ull) return false;   // (the bytes on record are fewer than the block: no parity word to read)
  return v.pass(ch.h_payload.data() + payload_off, tbs);
}

}  // namespace lsn

// lsn_front_launch.cc - the front end's launches on the host side: lsn_launch_front, the one launcher of a cell's filter-and-resampler
// chain (lsn_front_launch.h), and the stand-alone entry points, which need no Phy (like lsn_cell_search): lsn_resample, lsn_resample_cells[_ring] run the resampler
// alone, lsn_channel_filter[_ring] the channel filter alone.  Each of those is ONE launch of ONE stage - not the chain - between the staging of its input and its
// outputs, which Staging does for all of them.  Product code: no CPU fallback (the kernels alone compute the samples), nothing from oracle/ is included or linked.
#include "lsn_hip.h"
#include "../kernels/lsn_dev.h"
#include "lsn_front_launch.h"
#include <algorithm>
#include <cstdio>
#include <vector>

void lsn::lsn_launch_front(const LsnFrontSource& src, const FrontCell* const* cells, const LsnResampleCell* k, const int64_t* lo, const int64_t* hi, uint32_t n, hipStream_t s,
                           const char* what)
{
  if (!n || n > LSN_FILE_MAX_CELLS) throw std::runtime_error("front end: bad number of cells");
  if (!cells[0]->filtered()) {
    if (n == 1 && !src.ring_samples) lsn_launch_resample(src, k[0], s);
    else lsn_launch_resample_cells(src, k, n, s);
    return;
  }
  LsnChanFirCell f[LSN_FILE_MAX_CELLS];
  int64_t lo2[LSN_FILE_MAX_CELLS], hi2[LSN_FILE_MAX_CELLS];
  for (uint32_t c = 0; c < n; c++) {
    f[c] = LsnChanFirCell();
    if (!k[c].n_out) continue;
    const FrontCell& q = *cells[c];
    if (!chan_mid_span(lo[c], hi[c], q.mid_cap, lo2[c], hi2[c])) throw std::runtime_error(std::string(what) + "'s filtered samples do not fit the intermediate buffer");
    f[c] = q.ft.cell(*q.cf, q.mid, lo2[c], (uint64_t)(hi2[c] - lo2[c]));
  }
  lsn_launch_chan_fir(src, f, n, s);
  // stage 2 reads cf32 that the mixer has been through: the piece's plan was formed with no centre offset (tune = 0, no NCO tables)
  for (uint32_t c = 0; c < n; c++)
    if (k[c].n_out) lsn_launch_resample({cells[c]->mid, 0, 1.0f, lo2[c], (uint64_t)(hi2[c] - lo2[c]), src.nant, 0}, k[c], s);
}

namespace {

// what a stand-alone call puts on the device, given back with its scope: a stream, the input, the outputs of up to LSN_FILE_MAX_CELLS cells
struct Staging {
  lsn::OwnedStream st;
  // a host input of `bytes` bytes, staged as it lies; an input on the device (or an empty one) stays where it is
  const void* input(const void* src, bool on_device, size_t bytes)
  {
    if (on_device || !bytes) return src;
    void* d = in.alloc<uint8_t>(bytes);
    HIP_CHECK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st));
    return d;
  }
  // the whole host window [in_base, in_base + n_in) of samples of smp bytes at its slots in a ring of ring_samples samples.  Slots no sample of the window goes to
  // keep a pattern (NaN as cf32) that a read outside the window would carry into the outputs
  const void* ring(const void* src, uint64_t in_base, uint64_t n_in, uint64_t ring_samples, size_t smp)
  {
    uint8_t* d = in.alloc<uint8_t>(ring_samples * smp);
    HIP_CHECK(hipMemsetAsync(d, 0xFF, ring_samples * smp, st));
    const uint64_t slot = in_base & (ring_samples - 1), head = std::min(n_in, ring_samples - slot);
    if (head) HIP_CHECK(hipMemcpyAsync(d + slot * smp, src, head * smp, hipMemcpyHostToDevice, st));
    if (n_in > head) HIP_CHECK(hipMemcpyAsync(d, (const uint8_t*)src + head * smp, (n_in - head) * smp, hipMemcpyHostToDevice, st));   // behind the end of the ring
    return d;
  }
  // where the launch writes cell c's n samples of nant antennas: a device buffer that finish() copies to the host output, or the output itself when it is on the device
  cf32* output(uint32_t c, float* out, bool on_device, uint64_t n, uint32_t nant)
  {
    const size_t bytes = (size_t)n * nant * sizeof(cf32);
    if (on_device || !bytes) return (cf32*)out;
    outs[c].host = out; outs[c].bytes = bytes;
    return (cf32*)outs[c].dev.alloc<uint8_t>(bytes);
  }
  // the copies back and the ONE synchronise
  void finish()
  {
    for (auto& o : outs)
      if (o.bytes) HIP_CHECK(hipMemcpyAsync(o.host, o.dev.p, o.bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }

private:
  lsn::DevBuf in;
  struct { lsn::DevBuf dev; float* host = nullptr; size_t bytes = 0; } outs[LSN_FILE_MAX_CELLS];
};

// body(staging) on `device`, then the copies back; an exception on the way is one line on stderr under the call's name and LSN_ERROR.  The tables a body's launch
// reads are declared in front of this call: they outlive finish()
template <class F>
int staged(const char* name, int device, F&& body)
{
  try {
    HIP_CHECK(hipSetDevice(device));
    Staging g;
    body(g);
    g.finish();
    return LSN_SUCCESS;
  } catch (const std::exception& ex) {
    fprintf(stderr, "ltesniffer_amd: %s: %s\n", name, ex.what());
    return LSN_ERROR;
  }
}

}  // namespace

extern "C" {

int lsn_resample(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_resample_cfg_t* cfg, float* out, int out_on_device, uint64_t n_out)
{
  lsn::ResamplePlan plan;
  const int r = lsn_resample_plan(cfg, plan);
  if (r != LSN_SUCCESS) return r;
  if (!n_out) return LSN_SUCCESS;
  if (!in || !out || n_out >= (1ull << 32) || cfg->out_first >= (1ull << 40) || cfg->in_base >= (1ull << 62) || n_in >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  int64_t lo, hi;
  plan.inputSpan(cfg->out_first, n_out, lo, hi);
  if (hi >= (int64_t)1 << 62) return LSN_ERROR_INVALID_INPUTS;
  const LsnWindowNeed need = lsn_window_holds(cfg->in_base, n_in, lo, hi);
  if (!need.ok) return LSN_ERROR_INVALID_INPUTS;
  const uint32_t nant = cfg->nof_antennas, fmt = cfg->sample_format;
  const LsnSampleFormat sfm = lsn_sample_format(fmt, cfg->sample_scale);
  const size_t smp = (size_t)sfm.bytes * nant;
  const uint8_t* src = (const uint8_t*)in + ((uint64_t)need.lo - cfg->in_base) * smp;
  lsn::ResampleTables tb;
  return staged("resample", device, [&](Staging& g) {
    tb.upload(plan, g.st);
    const void* raw = g.input(src, in_on_device, need.len * smp);
    lsn_launch_resample({raw, fmt, sfm.scale, need.lo, need.len, nant, 0}, plan.cell(cfg->out_first, (uint32_t)n_out, tb, g.output(0, out, out_on_device, n_out, nant), n_out), g.st);
  });
}

// several resamplings of one input: one upload of the union of what the cells read, one launch of k_resample_cells.  ring_samples != 0 (host input): the whole
// window goes to its slots in a device ring of that many samples instead, and k_resample_ring reads it there
static_assert(LSN_RS_MAP_MAX_OUT == LSN_MAP_MAX_OUT, "lsn_resample.h speaks the public header's limit");

// maps (lsn_resample_cells[_ring]_map; null: none): cell c with maps[c].nof_out != 0 is cut through its antenna map and writes nof_out rows
static int resample_cells(int device, const void* in, int in_on_device, uint64_t n_in, uint64_t ring_samples, const lsn_resample_cfg_t* cfgs, const lsn_antenna_map_t* maps,
                          uint32_t n_cells, float* const* outs, int out_on_device, const uint64_t* n_out)
{
  if (!cfgs || !outs || !n_out || n_cells < 1 || n_cells > LSN_FILE_MAX_CELLS) return LSN_ERROR_INVALID_INPUTS;
  std::vector<lsn::ResamplePlan> plans(n_cells);
  const lsn_resample_cfg_t& c0 = cfgs[0];
  int64_t need_lo = 0, need_hi = 0;
  bool any = false;
  for (uint32_t c = 0; c < n_cells; c++) {
    const lsn_resample_cfg_t& k = cfgs[c];
    const int r = lsn_resample_plan_map(&k, maps ? &maps[c] : nullptr, plans[c]);
    if (r != LSN_SUCCESS) return r;
    if (k.struct_size != sizeof(lsn_resample_cfg_t) || k.nof_antennas != c0.nof_antennas || k.sample_format != c0.sample_format || !(k.sample_scale == c0.sample_scale) ||
        k.rate_in_hz != c0.rate_in_hz || k.in_base != c0.in_base)
      return LSN_ERROR_INVALID_INPUTS;
    if (!n_out[c]) continue;
    if (!in || !outs[c] || n_out[c] >= (1ull << 32) || k.out_first >= (1ull << 40) || k.in_base >= (1ull << 62) || n_in >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
    int64_t lo, hi;
    plans[c].inputSpan(k.out_first, n_out[c], lo, hi);
    if (hi >= (int64_t)1 << 62) return LSN_ERROR_INVALID_INPUTS;
    const LsnWindowNeed need = lsn_window_holds(k.in_base, n_in, lo, hi);
    if (!need.ok) return LSN_ERROR_INVALID_INPUTS;
    lo = need.lo;
    need_lo = any ? std::min(need_lo, lo) : lo;
    need_hi = any ? std::max(need_hi, hi) : hi;
    any = true;
  }
  if (!any) return LSN_SUCCESS;
  const uint32_t nant = c0.nof_antennas, fmt = c0.sample_format;
  const LsnSampleFormat sfm = lsn_sample_format(fmt, c0.sample_scale);
  const size_t smp = (size_t)sfm.bytes * nant;
  const uint64_t len = need_hi > need_lo ? (uint64_t)(need_hi - need_lo) : 0;
  const uint8_t* src = (const uint8_t*)in + ((uint64_t)need_lo - c0.in_base) * smp;
  std::vector<lsn::ResampleTables> tb(n_cells);
  return staged("resample_cells", device, [&](Staging& g) {
    const LsnFrontSource from = ring_samples ? LsnFrontSource{g.ring(in, c0.in_base, n_in, ring_samples, smp), fmt, sfm.scale, (int64_t)c0.in_base, n_in, nant, ring_samples}
                                                : LsnFrontSource{g.input(src, in_on_device, len * smp), fmt, sfm.scale, need_lo, len, nant, 0};
    LsnResampleCell k[LSN_FILE_MAX_CELLS];
    for (uint32_t c = 0; c < n_cells; c++) {
      tb[c].upload(plans[c], g.st);
      k[c] = plans[c].cell(cfgs[c].out_first, (uint32_t)std::max<uint64_t>(n_out[c], 1), tb[c],
                           g.output(c, outs[c], out_on_device, n_out[c], plans[c].map_nout ? plans[c].map_nout : nant), n_out[c]);
    }
    lsn_launch_resample_cells(from, k, n_cells, g.st);
  });
}

int lsn_resample_cells(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_resample_cfg_t* cfgs, uint32_t n_cells, float* const* outs, int out_on_device,
                       const uint64_t* n_out)
{
  return resample_cells(device, in, in_on_device, n_in, 0, cfgs, nullptr, n_cells, outs, out_on_device, n_out);
}

int lsn_resample_cells_map(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_resample_cfg_t* cfgs, const lsn_antenna_map_t* maps, uint32_t n_cells,
                           float* const* outs, int out_on_device, const uint64_t* n_out)
{
  if (!maps) return LSN_ERROR_INVALID_INPUTS;
  return resample_cells(device, in, in_on_device, n_in, 0, cfgs, maps, n_cells, outs, out_on_device, n_out);
}

int lsn_resample_cells_ring(int device, const void* in, uint64_t n_in, uint64_t ring_samples, const lsn_resample_cfg_t* cfgs, uint32_t n_cells, float* const* outs,
                            const uint64_t* n_out)
{
  if (!in || !lsn_ring_holds(ring_samples, n_in)) return LSN_ERROR_INVALID_INPUTS;
  return resample_cells(device, in, 0, n_in, ring_samples, cfgs, nullptr, n_cells, outs, 0, n_out);
}

int lsn_resample_cells_ring_map(int device, const void* in, uint64_t n_in, uint64_t ring_samples, const lsn_resample_cfg_t* cfgs, const lsn_antenna_map_t* maps,
                                uint32_t n_cells, float* const* outs, const uint64_t* n_out)
{
  if (!in || !maps || !lsn_ring_holds(ring_samples, n_in)) return LSN_ERROR_INVALID_INPUTS;
  return resample_cells(device, in, 0, n_in, ring_samples, cfgs, maps, n_cells, outs, 0, n_out);
}

// stage 1 alone (k_chan_fir)
int lsn_channel_filter(int device, const void* in, int in_on_device, uint64_t n_in, const lsn_channel_filter_cfg_t* cfg, float* out, int out_on_device, uint64_t n_out)
{
  lsn::ChanFilter f;
  const int r = lsn_channel_filter_plan(cfg, f);
  if (r != LSN_SUCCESS) return r;
  if (!n_out) return LSN_SUCCESS;
  if (!in || !out || n_out >= (1ull << 40) || n_in >= (1ull << 62)) return LSN_ERROR_INVALID_INPUTS;
  int64_t lo = (int64_t)cfg->out_first, hi = (int64_t)(cfg->out_first + n_out);
  f.widen(lo, hi);
  const LsnWindowNeed need = lsn_window_holds(cfg->in_base, n_in, lo, hi);
  if (!need.ok) return LSN_ERROR_INVALID_INPUTS;
  const uint32_t nant = cfg->nof_antennas, fmt = cfg->sample_format;
  const LsnSampleFormat sfm = lsn_sample_format(fmt, cfg->sample_scale);
  const size_t smp = (size_t)sfm.bytes * nant;
  const uint8_t* src = (const uint8_t*)in + ((uint64_t)need.lo - cfg->in_base) * smp;
  lsn::ChanFirTables ft;
  return staged("channel_filter", device, [&](Staging& g) {
    ft.upload(f, g.st);
    const void* raw = g.input(src, in_on_device, need.len * smp);
    const LsnChanFirCell k = ft.cell(f, g.output(0, out, out_on_device, n_out, nant), (int64_t)cfg->out_first, n_out);
    lsn_launch_chan_fir({raw, fmt, sfm.scale, need.lo, need.len, nant, 0}, &k, 1, g.st);
  });
}

// stage 1 out of a ring (k_chan_fir_ring): the whole window goes to its slots of a device ring, every cell's filter runs in ONE launch
int lsn_channel_filter_ring(int device, const void* in, uint64_t n_in, uint64_t ring_samples, const lsn_channel_filter_cfg_t* cfgs, uint32_t n_cells, float* const* outs,
                            const uint64_t* n_out)
{
  if (!in || !cfgs || !outs || !n_out || n_cells < 1 || n_cells > LSN_FILE_MAX_CELLS) return LSN_ERROR_INVALID_INPUTS;
  if (!lsn_ring_holds(ring_samples, n_in)) return LSN_ERROR_INVALID_INPUTS;
  std::vector<lsn::ChanFilter> f(n_cells);
  const lsn_channel_filter_cfg_t& c0 = cfgs[0];
  bool any = false;
  for (uint32_t c = 0; c < n_cells; c++) {
    const lsn_channel_filter_cfg_t& k = cfgs[c];
    const int r = lsn_channel_filter_plan(&k, f[c]);
    if (r != LSN_SUCCESS) return r;
    if (k.nof_antennas != c0.nof_antennas || k.sample_format != c0.sample_format || !(k.sample_scale == c0.sample_scale) || k.rate_in_hz != c0.rate_in_hz || k.in_base != c0.in_base)
      return LSN_ERROR_INVALID_INPUTS;
    if (!n_out[c]) continue;
    if (!outs[c] || n_out[c] >= (1ull << 40)) return LSN_ERROR_INVALID_INPUTS;
    int64_t lo = (int64_t)k.out_first, hi = (int64_t)(k.out_first + n_out[c]);
    f[c].widen(lo, hi);
    if (!lsn_window_holds(k.in_base, n_in, lo, hi).ok) return LSN_ERROR_INVALID_INPUTS;
    any = true;
  }
  if (!any) return LSN_SUCCESS;
  const uint32_t nant = c0.nof_antennas, fmt = c0.sample_format;
  const LsnSampleFormat sfm = lsn_sample_format(fmt, c0.sample_scale);
  std::vector<lsn::ChanFirTables> ft(n_cells);
  return staged("channel_filter_ring", device, [&](Staging& g) {
    const void* d_ring = g.ring(in, c0.in_base, n_in, ring_samples, (size_t)sfm.bytes * nant);
    LsnChanFirCell k[LSN_FILE_MAX_CELLS];
    for (uint32_t c = 0; c < n_cells; c++) {
      k[c] = LsnChanFirCell();
      if (!n_out[c]) continue;
      ft[c].upload(f[c], g.st);
      k[c] = ft[c].cell(f[c], g.output(c, outs[c], 0, n_out[c], nant), (int64_t)cfgs[c].out_first, n_out[c]);
    }
    lsn_launch_chan_fir({d_ring, fmt, sfm.scale, (int64_t)c0.in_base, n_in, nant, ring_samples}, k, n_cells, g.st);
  });
}

}  // extern "C"

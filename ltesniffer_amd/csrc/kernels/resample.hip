// resample.hip - polyphase Kaiser-windowed-sinc resampler of the file source and of lsn_resample (gfx950).  The filter, the bank and the
// position arithmetic are defined in DESIGN.md section 3.1b; the host side (plan, bank, spans, the launch record of a cell) is host/lsn_resample.{h,cc}, and
// the launchers at the end of this file take that record as it is.
//
// Output sample m of a replay sits at input position P0 + m * D, a 64.64 fixed-point number (integer part = input sample index, 64 bits of
// fraction).  The launch is handed the position of ITS first output (base = P0 + m0 * D, formed on the host in 128-bit integers) and D; a
// lane forms i * D with a 64 x 64 -> 128 multiply and adds.  Integer arithmetic throughout: an output is a function of the input, the
// configuration and m alone - not of the block, the run or the launch it was computed in.
//
// One workgroup produces LSN_RS_RUN consecutive outputs of one antenna.  It stages the input span of the run (floor(RUN * D) + T + 1
// samples, converted to float while loading, zeros in front of input sample 0 and outside the buffer) in LDS as [sample] float2, then every
// lane runs the T taps of its outputs: coefficient j = H[p][j] + f * dH[p][j] (p = top 9 bits of the fraction, f = the next 24 bits), one
// 16-byte load of the bank row gives two taps, one ds_read_b64 per sample.  Up-sampling and equal rates: neighbouring lanes read the
// same or neighbouring float2 (broadcast / conflict free); down-sampling by r strides the lanes by r float2 = a 2- to 4-way conflict.
//
// MIX instantiations (a cell off the recording's centre, DESIGN 3.1b "Frequency translation"): input sample n is multiplied by
// exp(-2 pi j Phi(n) / 2^64), Phi(n) = n * W mod 2^64 with n the sample's index in the RECORDING, while it is staged - the one place every input
// sample is touched once; the tap loop does not know.  The exponential is the two-table NCO of k_ofdm (4096 coarse x 1024 fine entries).
//
// Three kernels expand the one copy of that text: k_resample (one cell, a linear buffer), k_resample_cells (several cells, one linear buffer) and
// k_resample_ring (several cells out of the device ring a pushed stream keeps its raw samples in).
#include "lsn_front_dev.h"
#include "../host/lsn_resample_launch.h"
#include <algorithm>
#include <cstring>

#define LSN_RS_RUN 512u      // outputs per workgroup (256 lanes x 2)

struct LsnResampleArgs {
  const void* raw;       // input, [sample][antenna], element 0 = input sample buf_base of the recording
  int64_t buf_base;      // >= 0
  uint64_t buf_len;      // samples (per antenna) in raw
  uint64_t base_hi, base_lo;  // position of the launch's output 0
  uint64_t d_lo;         // D: fraction ...
  uint32_t d_hi;         // ... and integer part (0 .. 4)
  uint32_t taps;         // T, even
  uint32_t span;         // samples staged per run (the LDS request is span * 8 bytes)
  uint32_t nant;
  uint32_t sflen;        // outputs per antenna row: launch output i goes to out[((i / sflen) * nant + a) * sflen + i % sflen]
  uint32_t sf_off;       // phase of launch output 0 inside its row (0 for the file source: launches start on a subframe)
  uint64_t n_out;        // outputs of the launch, per antenna
  float scale;
  uint32_t ring_mask;    // k_resample_ring: raw is a ring of ring_mask + 1 samples (a power of two), recording sample n sits at slot n & ring_mask; else 0 and unread
  const float2* bank;    // [512][T] (H, dH)
  const cf32* rot;       // optional [sflen]
  cf32* out;
  uint64_t w;            // MIX: tuning word W ...
  const cf32* nco;       // ... and the NCO tables, [4096] coarse then [1024] fine
};
static_assert(sizeof(LsnResampleArgs) == 128, "eight of them are one kernel argument block; ring_mask sits in what was padding behind scale");

// One run of one antenna: the staging loop and the tap loop.  They exist ONCE in this file, as text: the body is a macro that the kernels expand, over the names A
// (the run's LsnResampleArgs), rs_x (the dynamic LDS) and FMT (why a macro and not a function: lsn_front_dev.h, whose staged sample and position arithmetic these
// are).  Two things differ between the kernels: MIXCOND - k_resample's template flag, or the cell's own "has NCO tables", uniform over the workgroup - and SRCSAMPLE,
// where the sample sits in A.raw: k_resample and k_resample_cells read a linear buffer (LSN_FRONT_LINEAR), k_resample_ring the slot of n in its ring (LSN_FRONT_RING).
// The staging loop, from the position of the run's first output to the barrier, is the one text of both run geometries; RUNLEN is the outputs of a run.
// Three more things are one number, blockIdx.y, in these kernels and three numbers in the antenna-map kernels further down: SRCANT, the antenna of the
// recording's A.nant a workgroup reads; OUTROW of OUTROWS, the row it writes; TUNE, its tuning word.  The kernels here pass blockIdx.y, a of A.nant and A.w - the text
// they had before the parameters existed, and the instruction streams.
#define LSN_RESAMPLE_STAGE(RUNLEN, MIXCOND, SRCSAMPLE, SRCANT, TUNE) \
  const uint32_t a = SRCANT, half = A.taps / 2;                                                                                                                         \
  const uint64_t i0 = (uint64_t)blockIdx.x * (RUNLEN);                                                                                                                  \
  LSN_FRONT_POSITION(i0, hi, lo)  /* of the run's first output */                                                                                                       \
  const int64_t n_lo = (int64_t)hi - (int64_t)half + 1;  /* input sample staged at rs_x[0] */                                                                           \
  for (uint32_t s = threadIdx.x; s < A.span; s += 256) {                                                                                                                \
    LSN_FRONT_SAMPLE(true, SRCSAMPLE, MIXCOND, TUNE)                                                                                                                    \
    rs_x[s] = x;                                                                                                                                                        \
  }                                                                                                                                                                     \
  __syncthreads();

#define LSN_RESAMPLE_RUN(MIXCOND, SRCSAMPLE, SRCANT, TUNE, OUTROW, OUTROWS) \
  LSN_RESAMPLE_STAGE(LSN_RS_RUN, MIXCOND, SRCSAMPLE, SRCANT, TUNE)                                                                                                      \
  for (uint32_t r = 0; r < LSN_RS_RUN / 256; r++) {                                                                                                                     \
    const uint64_t i = i0 + r * 256 + threadIdx.x;                                                                                                                      \
    if (i >= A.n_out) break;                                                                                                                                            \
    LSN_FRONT_POSITION(i, phi, plo)                                                                                                                                     \
    const uint32_t s0 = (uint32_t)((int64_t)phi - (int64_t)half + 1 - n_lo);  /* first of the T staged samples of this output */                                        \
    LSN_FRONT_PHASE(plo, p, f)                                                                                                                                          \
    if (s0 + A.taps > A.span) continue;  /* cannot happen (the host sizes span); keeps the LDS reads inside */                                                          \
    const float4* row = (const float4*)(A.bank + (size_t)p * A.taps);                                                                                                   \
    const float2* x = rs_x + s0;                                                                                                                                        \
    float yr = 0.0f, yi = 0.0f;                                                                                                                                         \
    for (uint32_t j = 0; j < half; j++) {                                                                                                                               \
      const float4 c = row[j];                                                                                                                                          \
      const float c0 = __builtin_fmaf(f, c.y, c.x), c1 = __builtin_fmaf(f, c.w, c.z);                                                                                   \
      const float2 x0 = x[2 * j], x1 = x[2 * j + 1];                                                                                                                    \
      yr = __builtin_fmaf(c0, x0.x, yr); yi = __builtin_fmaf(c0, x0.y, yi);                                                                                             \
      yr = __builtin_fmaf(c1, x1.x, yr); yi = __builtin_fmaf(c1, x1.y, yi);                                                                                             \
    }                                                                                                                                                                   \
    const uint32_t q = (uint32_t)i + A.sf_off, sf = q / A.sflen, n = q - sf * A.sflen;  /* the launcher keeps n_out + sf_off below 2^32 */                              \
    cf32 y; y.r = yr; y.i = yi;                                                                                                                                         \
    if (A.rot) y = cmul(y, A.rot[n]);                                                                                                                                   \
    A.out[((size_t)sf * (OUTROWS) + (OUTROW)) * A.sflen + n] = y;                                                                                                             \
  }

template <int FMT, bool MIX>
__global__ __launch_bounds__(256) void k_resample(const LsnResampleArgs A)
{
  extern __shared__ float2 rs_x[];
  LSN_RESAMPLE_RUN(MIX, LSN_FRONT_LINEAR, blockIdx.y, A.w, a, A.nant)
}

// Several cells of one recording from ONE raw buffer in one launch (lsn_file_process_cells, lsn_resample_cells): grid (largest number of runs
// of a cell, antennas, cells).  The cells' arguments travel in the kernel argument block (8 x 128 bytes) and are read with scalar loads - the cell index is
// blockIdx.z, the same for every lane.  Cells differ in D, T, n_out, sflen, bank and output buffer, so a workgroup in front of which its cell has no run left is
// the normal case: it returns before it touches LDS.  The dynamic LDS request is the largest span of the launch's cells.  A cell mixes when it has NCO tables.
#define LSN_RS_MAX_CELLS 8u
struct LsnResampleCellsArgs { LsnResampleArgs c[LSN_RS_MAX_CELLS]; };

template <int FMT>
__global__ __launch_bounds__(256) void k_resample_cells(const LsnResampleCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleArgs& A = P.c[blockIdx.z];
  if ((uint64_t)blockIdx.x * LSN_RS_RUN >= A.n_out) return;
  LSN_RESAMPLE_RUN(A.nco != nullptr, LSN_FRONT_LINEAR, blockIdx.y, A.w, a, A.nant)
}

// The same launch out of a RING (lsn_stream, lsn_resample_cells_ring): raw holds ring_mask + 1 samples per antenna and sample n of the recording sits
// at slot n & ring_mask, wherever the pushes that brought it were cut.  Grid, argument block and early exit are k_resample_cells'; a source index is below
// (ring_mask + 1) * nant whatever n is, and the window test in front of it keeps a run from staging a slot that holds another lap's sample.
template <int FMT>
__global__ __launch_bounds__(256) void k_resample_ring(const LsnResampleCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleArgs& A = P.c[blockIdx.z];
  if ((uint64_t)blockIdx.x * LSN_RS_RUN >= A.n_out) return;
  LSN_RESAMPLE_RUN(A.nco != nullptr, LSN_FRONT_RING, blockIdx.y, A.w, a, A.nant)
}

// ---- ratios above 4: the wide-ratio run ----
//
// Above ratio 4 one lane per output strides the lanes' LDS reads by the ratio (a 32-way conflict at ratio 32) and a run of 512 outputs no longer fits LDS.  Here
// GRP lanes (8, 16 or 32: the smallest power of two >= the plan's NOMINAL ratio, which is at most 32 - fixed when the plan is made, never the launch's or a
// tracked segment's choice) share one output: lane q of a group sums taps j = q, q + GRP, q + 2 GRP, ... (j < T; T is no multiple of GRP in general) in ascending j
// into its own accumulator, and the GRP partial sums are added by an xor butterfly in the fixed order GRP/2 .. 1, after which every lane of the group holds the
// same bits.  An output is therefore still a function of (input samples, configuration, m) alone: which taps meet in which accumulator, and in what order the
// accumulators are added, depends on j, T and GRP and on nothing else.  In one step of the tap loop the lanes of a group read GRP consecutive float2 of LDS
// (one ds_read_b64 each) and GRP consecutive float2 (H, dH) of the bank row; neighbouring groups start floor-of-ratio float2 apart, and because GRP >= ratio
// the 32 lanes of a half wavefront stay inside 32 consecutive float2 = the 64 banks of ds_read_b64 once (overlapping groups read the SAME addresses:
// broadcast).  A workgroup runs W.run / (256 / GRP) = 16 rounds of 256 / GRP outputs over one staged span of floor(run * D) + T + 2 <= 4096 + 770 samples.
// The staging loop is LSN_RESAMPLE_RUN's - the same LSN_RESAMPLE_STAGE - and the position arithmetic the same lsn_front_dev.h; c_j = fma(f, dH, H) and the one
// fma per product are as there.
struct LsnResampleWideArgs {
  LsnResampleArgs a;
  uint32_t grp, run;     // lanes per output (8, 16, 32) and outputs per workgroup (4096 / grp)
};
static_assert(sizeof(LsnResampleWideArgs) == 136, "eight of them are one kernel argument block");

#define LSN_RESAMPLE_WIDE_RUN(MIXCOND, SRCSAMPLE, SRCANT, TUNE, OUTROW, OUTROWS) \
  LSN_RESAMPLE_STAGE(W.run, MIXCOND, SRCSAMPLE, SRCANT, TUNE)                                                                                                           \
  const uint32_t per = 256u / W.grp, gi = threadIdx.x / W.grp, gq = threadIdx.x & (W.grp - 1u);  /* outputs per round; this lane's output in it and lane in its group */ \
  for (uint32_t r = 0; r * per < W.run; r++) {                                                                                                                          \
    if (i0 + r * per >= A.n_out) break;  /* uniform over the workgroup: no output of this or a later round exists */                                                    \
    const uint64_t i = i0 + r * per + gi;                                                                                                                               \
    LSN_FRONT_POSITION(i, phi, plo)                                                                                                                                     \
    const uint32_t s0 = (uint32_t)((int64_t)phi - (int64_t)half + 1 - n_lo);  /* first of the T staged samples of this output */                                        \
    LSN_FRONT_PHASE(plo, p, f)                                                                                                                                          \
    /* s0 + T > span cannot happen for an output that exists (the host sizes span); the test keeps the LDS reads inside.  Every lane of a group agrees on it */         \
    const bool live = i < A.n_out && s0 <= A.span && s0 + A.taps <= A.span;                                                                                             \
    float yr = 0.0f, yi = 0.0f;                                                                                                                                         \
    if (live) {                                                                                                                                                         \
      const float2* row = A.bank + (size_t)p * A.taps;                                                                                                                  \
      const float2* x = rs_x + s0;                                                                                                                                      \
      uint32_t j = gq;                                                                                                                                                  \
      /* four taps of this lane at a time while all four exist: eight loads in flight, the same fmas in the same (ascending j) order as the loop behind it */           \
      for (; j + 3u * W.grp < A.taps; j += 4u * W.grp) {                                                                                                                \
        const float2 ca = row[j], cb = row[j + W.grp], cc = row[j + 2u * W.grp], cd = row[j + 3u * W.grp];                                                              \
        const float2 xa = x[j], xb = x[j + W.grp], xc = x[j + 2u * W.grp], xd = x[j + 3u * W.grp];                                                                      \
        const float ja = __builtin_fmaf(f, ca.y, ca.x), jb = __builtin_fmaf(f, cb.y, cb.x), jc = __builtin_fmaf(f, cc.y, cc.x), jd = __builtin_fmaf(f, cd.y, cd.x);     \
        yr = __builtin_fmaf(ja, xa.x, yr); yi = __builtin_fmaf(ja, xa.y, yi);                                                                                           \
        yr = __builtin_fmaf(jb, xb.x, yr); yi = __builtin_fmaf(jb, xb.y, yi);                                                                                           \
        yr = __builtin_fmaf(jc, xc.x, yr); yi = __builtin_fmaf(jc, xc.y, yi);                                                                                           \
        yr = __builtin_fmaf(jd, xd.x, yr); yi = __builtin_fmaf(jd, xd.y, yi);                                                                                           \
      }                                                                                                                                                                 \
      for (; j < A.taps; j += W.grp) {                                                                                                                                  \
        const float2 c = row[j], xj = x[j];                                                                                                                             \
        const float cj = __builtin_fmaf(f, c.y, c.x);                                                                                                                   \
        yr = __builtin_fmaf(cj, xj.x, yr); yi = __builtin_fmaf(cj, xj.y, yi);                                                                                           \
      }                                                                                                                                                                 \
    }                                                                                                                                                                   \
    /* every lane takes part: a lane's partners are the lanes of its own group (m < grp), live or not together */                                                       \
    for (uint32_t m = W.grp >> 1; m; m >>= 1) {                                                                                                                         \
      yr += __shfl_xor(yr, (int)m); yi += __shfl_xor(yi, (int)m);                                                                                                       \
    }                                                                                                                                                                   \
    if (live && gq == 0) {                                                                                                                                              \
      const uint32_t q = (uint32_t)i + A.sf_off, sf = q / A.sflen, n = q - sf * A.sflen;  /* the launcher keeps n_out + sf_off below 2^32 */                            \
      cf32 y; y.r = yr; y.i = yi;                                                                                                                                       \
      if (A.rot) y = cmul(y, A.rot[n]);                                                                                                                                 \
      A.out[((size_t)sf * (OUTROWS) + (OUTROW)) * A.sflen + n] = y;                                                                                                           \
    }                                                                                                                                                                   \
  }

template <int FMT, bool MIX>
__global__ __launch_bounds__(256) void k_resample_wide(const LsnResampleWideArgs W)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleArgs& A = W.a;
  LSN_RESAMPLE_WIDE_RUN(MIX, LSN_FRONT_LINEAR, blockIdx.y, A.w, a, A.nant)
}

struct LsnResampleWideCellsArgs { LsnResampleWideArgs c[LSN_RS_MAX_CELLS]; };

// the wide-ratio cells of a launch of lsn_launch_resample_cells: grid, early exit and "a cell mixes when it has NCO tables" as k_resample_cells
template <int FMT>
__global__ __launch_bounds__(256) void k_resample_cells_wide(const LsnResampleWideCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleWideArgs& W = P.c[blockIdx.z];
  const LsnResampleArgs& A = W.a;
  if ((uint64_t)blockIdx.x * W.run >= A.n_out) return;
  LSN_RESAMPLE_WIDE_RUN(A.nco != nullptr, LSN_FRONT_LINEAR, blockIdx.y, A.w, a, A.nant)
}

// ... and out of a ring, as k_resample_ring
template <int FMT>
__global__ __launch_bounds__(256) void k_resample_ring_wide(const LsnResampleWideCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleWideArgs& W = P.c[blockIdx.z];
  const LsnResampleArgs& A = W.a;
  if ((uint64_t)blockIdx.x * W.run >= A.n_out) return;
  LSN_RESAMPLE_WIDE_RUN(A.nco != nullptr, LSN_FRONT_RING, blockIdx.y, A.w, a, A.nant)
}

// ---- the antenna map ----
//
// The kernels above read antenna blockIdx.y of the recording, write row blockIdx.y of as many rows, and tune by the cell's one word.  With a map the three are
// separate: a workgroup READS antenna src[blockIdx.y] of the recording's A.nant, WRITES row blockIdx.y of the cell's `rows`, and tunes by w[blockIdx.y] - a word of
// 0 is not mixed; the test is uniform over the workgroup.  Grid: runs x the largest number of OUTPUT rows of a cell x cells; one cell is a launch of grid.z = 1.
// The per-cell map travels in the argument block behind the cells' arguments and is read with scalar loads.  The run text, LDS, the tap loop and the 64.64
// arithmetic are the macros above: output row a equals row src[a] of the unmapped kernel run with the word w[a], bit for bit.  A cell without a map takes part in
// such a launch as the identity - src[a] = a, w[a] = its word, rows = the recording's antennas -, hence eight entries.
#define LSN_RS_MAP_ROWS 8u
struct LsnResampleMap {
  uint32_t rows, pad;              // rows the cell writes (a workgroup with blockIdx.y >= rows returns); at most LSN_RS_MAP_ROWS
  uint32_t src[LSN_RS_MAP_ROWS];   // < A.nant
  uint64_t w[LSN_RS_MAP_ROWS];     // != 0 only when A.nco is set
};
struct LsnResampleMapCellsArgs { LsnResampleArgs c[LSN_RS_MAX_CELLS]; LsnResampleMap m[LSN_RS_MAX_CELLS]; };
struct LsnResampleMapWideCellsArgs { LsnResampleWideArgs c[LSN_RS_MAX_CELLS]; LsnResampleMap m[LSN_RS_MAX_CELLS]; };
static_assert(sizeof(LsnResampleMapWideCellsArgs) <= 4096, "one kernel argument block");

#define LSN_RESAMPLE_MAP_ENTRY(RUNLEN)                                                                                                                                  \
  const LsnResampleMap& M = P.m[blockIdx.z];                                                                                                                            \
  if (blockIdx.y >= M.rows || (uint64_t)blockIdx.x * (RUNLEN) >= A.n_out) return;                                                                                       \
  const uint32_t orow = blockIdx.y;                                                                                                                                     \
  const uint64_t mw = M.w[orow];

template <int FMT>
__global__ __launch_bounds__(256) void k_resample_map(const LsnResampleMapCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleArgs& A = P.c[blockIdx.z];
  LSN_RESAMPLE_MAP_ENTRY(LSN_RS_RUN)
  LSN_RESAMPLE_RUN(mw != 0, LSN_FRONT_LINEAR, M.src[orow], mw, orow, M.rows)
}

template <int FMT>
__global__ __launch_bounds__(256) void k_resample_map_ring(const LsnResampleMapCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleArgs& A = P.c[blockIdx.z];
  LSN_RESAMPLE_MAP_ENTRY(LSN_RS_RUN)
  LSN_RESAMPLE_RUN(mw != 0, LSN_FRONT_RING, M.src[orow], mw, orow, M.rows)
}

template <int FMT>
__global__ __launch_bounds__(256) void k_resample_map_wide(const LsnResampleMapWideCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleWideArgs& W = P.c[blockIdx.z];
  const LsnResampleArgs& A = W.a;
  LSN_RESAMPLE_MAP_ENTRY(W.run)
  LSN_RESAMPLE_WIDE_RUN(mw != 0, LSN_FRONT_LINEAR, M.src[orow], mw, orow, M.rows)
}

template <int FMT>
__global__ __launch_bounds__(256) void k_resample_map_ring_wide(const LsnResampleMapWideCellsArgs P)
{
  extern __shared__ float2 rs_x[];
  const LsnResampleWideArgs& W = P.c[blockIdx.z];
  const LsnResampleArgs& A = W.a;
  LSN_RESAMPLE_MAP_ENTRY(W.run)
  LSN_RESAMPLE_WIDE_RUN(mw != 0, LSN_FRONT_RING, M.src[orow], mw, orow, M.rows)
}

// ---- host side: one function forms a run's arguments, two launchers (lsn_resample_launch.h) ----

// the map of cell k as its launch reads it, checked: a mapped cell's rows, sources (inside the recording's antennas) and words (non-zero only with NCO tables), or the
// identity over the recording's antennas.  -> the rows it writes
static uint32_t resample_map(const char* kernel, const LsnFrontSource& src, const LsnResampleCell& k, LsnResampleMap& M)
{
  memset(&M, 0, sizeof(M));
  if (src.nant < 1 || src.nant > LSN_RS_MAP_ROWS || k.map_nout > LSN_RS_MAP_MAX_OUT) throw std::runtime_error(std::string(kernel) + ": bad antenna map");
  if (!k.map_nout) {
    M.rows = src.nant;
    for (uint32_t a = 0; a < src.nant; a++) { M.src[a] = a; M.w[a] = k.nco ? k.w : 0; }
    return M.rows;
  }
  M.rows = k.map_nout;
  for (uint32_t a = 0; a < k.map_nout; a++) {
    if (k.map_src[a] >= src.nant || (k.map_w[a] && !k.nco)) throw std::runtime_error(std::string(kernel) + ": bad antenna map");
    M.src[a] = k.map_src[a]; M.w[a] = k.map_w[a];
  }
  return M.rows;
}

// the arguments of cell k's runs out of src, checked: span = samples a run needs (host: lsn_resample.cc), n_out + sf_off below 2^32 (the kernel's row arithmetic); a
// run is LSN_RS_RUN outputs, or k.run of the wide-ratio geometry (k.grp = 8, 16 or 32 lanes per output, k.run a whole number of rounds of 256 / k.grp).
// -> the cell's number of runs.  `kernel` names the launch in a refusal
static uint64_t resample_args(const char* kernel, const LsnFrontSource& src, const LsnResampleCell& k, LsnResampleArgs& A)
{
  if (k.taps < 2 || (k.taps & 1) || k.span < k.taps || (size_t)k.span * sizeof(float2) > 64 * 1024 || src.buf_base < 0 || !k.sflen)
    throw std::runtime_error(std::string(kernel) + ": bad geometry");
  if (k.grp && ((k.grp != 8 && k.grp != 16 && k.grp != 32) || !k.run || k.run % (256u / k.grp))) throw std::runtime_error(std::string(kernel) + ": bad geometry");
  const uint64_t run = k.grp ? k.run : LSN_RS_RUN, runs = (k.n_out + run - 1) / run;
  if (runs > 0x7FFFFFFFull || k.n_out + k.sf_off > 0xFFFFFFFFull) throw std::runtime_error(std::string(kernel) + ": launch too long");
  A.raw = src.raw; A.buf_base = src.buf_base; A.buf_len = src.buf_len; A.base_hi = k.base_hi; A.base_lo = k.base_lo; A.d_lo = k.d_lo; A.d_hi = k.d_hi; A.taps = k.taps; A.span = k.span;
  A.nant = src.nant; A.sflen = k.sflen; A.sf_off = k.sf_off; A.n_out = k.n_out; A.scale = src.scale; A.bank = (const float2*)k.bank; A.rot = k.rot; A.out = k.out;
  A.w = k.w; A.nco = k.nco; A.ring_mask = src.ring_samples ? (uint32_t)(src.ring_samples - 1) : 0;
  return runs;
}

// one cell out of a linear buffer.  cell.nco != null: the mixing instantiations with tuning word w; null: the plain ones, as before the mixer existed.  cell.grp != 0:
// the wide-ratio kernel
void lsn_launch_resample(const LsnFrontSource& src, const LsnResampleCell& cell, hipStream_t s)
{
  if (!cell.n_out) return;
  if (src.ring_samples) throw std::runtime_error("k_resample: reads a linear buffer");
  if (cell.map_nout) { lsn_launch_resample_cells(src, &cell, 1, s); return; }   // k_resample_map serves one cell too
  const size_t lds = (size_t)cell.span * sizeof(float2);
  if (cell.grp) {
    LsnResampleWideArgs W;
    memset(&W, 0, sizeof(W));
    const dim3 g((uint32_t)resample_args("k_resample_wide", src, cell, W.a), src.nant);
    W.grp = cell.grp; W.run = cell.run;
    if (cell.nco) LSN_LAUNCH_FMT(k_resample_wide, LSN_COMMA true, src.fmt, g, dim3(256), lds, s, W);
    else LSN_LAUNCH_FMT(k_resample_wide, LSN_COMMA false, src.fmt, g, dim3(256), lds, s, W);
    return;
  }
  LsnResampleArgs A;
  const dim3 g((uint32_t)resample_args("k_resample", src, cell, A), src.nant);
  if (cell.nco) LSN_LAUNCH_FMT(k_resample, LSN_COMMA true, src.fmt, g, dim3(256), lds, s, A);
  else LSN_LAUNCH_FMT(k_resample, LSN_COMMA false, src.fmt, g, dim3(256), lds, s, A);
}

// lsn_launch_resample_cells when a cell of the launch has an antenna map (the caller has checked ring and cell count): the same two launches - ratios up to 4, wide
// ratios - through the _map kernels, grid.y = the most rows a cell of the launch writes; an unmapped cell rides as the identity
static void launch_resample_map(const LsnFrontSource& src, const LsnResampleCell* cells, uint32_t n_cells, hipStream_t s)
{
  const uint64_t rn = src.ring_samples;
  const char* kernel = rn ? "k_resample_map_ring" : "k_resample_map";
  LsnResampleMapCellsArgs P;
  LsnResampleMapWideCellsArgs Q;
  memset(&P, 0, sizeof(P));
  memset(&Q, 0, sizeof(Q));
  uint32_t n = 0, span = 0, rows = 0, nw = 0, span_w = 0, rows_w = 0;
  uint64_t runs = 0, runs_w = 0;
  for (uint32_t c = 0; c < n_cells; c++) {
    if (!cells[c].n_out) continue;
    if (cells[c].grp) {
      LsnResampleWideArgs& W = Q.c[nw];
      runs_w = std::max(runs_w, resample_args(kernel, src, cells[c], W.a));
      W.grp = cells[c].grp; W.run = cells[c].run;
      span_w = std::max(span_w, cells[c].span);
      rows_w = std::max(rows_w, resample_map(kernel, src, cells[c], Q.m[nw++]));
    } else {
      runs = std::max(runs, resample_args(kernel, src, cells[c], P.c[n]));
      span = std::max(span, cells[c].span);
      rows = std::max(rows, resample_map(kernel, src, cells[c], P.m[n++]));
    }
  }
  if (n) {
    const dim3 g((uint32_t)runs, rows, n);
    const size_t lds = (size_t)span * sizeof(float2);
    if (!rn) LSN_LAUNCH_FMT(k_resample_map, , src.fmt, g, dim3(256), lds, s, P);
    else LSN_LAUNCH_FMT(k_resample_map_ring, , src.fmt, g, dim3(256), lds, s, P);
  }
  if (nw) {
    const dim3 g((uint32_t)runs_w, rows_w, nw);
    const size_t lds = (size_t)span_w * sizeof(float2);
    if (!rn) LSN_LAUNCH_FMT(k_resample_map_wide, , src.fmt, g, dim3(256), lds, s, Q);
    else LSN_LAUNCH_FMT(k_resample_map_ring_wide, , src.fmt, g, dim3(256), lds, s, Q);
  }
}

// the cells of one launch: the source is the recording's and shared, everything else is the cell's own.  A cell with n_out = 0 takes no part; no launch when
// none does.  Out of a ring: lsn_ring_holds(ring_samples, buf_len).  Cells of the two run geometries go to two launches on the same
// stream - the cells of ratio up to 4 to the kernel they always went to, with the arguments they always had; the wide-ratio cells to its _wide twin
void lsn_launch_resample_cells(const LsnFrontSource& src, const LsnResampleCell* cells, uint32_t n_cells, hipStream_t s)
{
  const uint64_t rn = src.ring_samples;
  const char* kernel = rn ? "k_resample_ring" : "k_resample_cells";
  if (rn && !lsn_ring_holds(rn, src.buf_len)) throw std::runtime_error("k_resample_ring: bad ring");
  if (n_cells > LSN_RS_MAX_CELLS || src.buf_base < 0) throw std::runtime_error(std::string(kernel) + ": bad geometry");
  bool mapped = false;
  for (uint32_t c = 0; c < n_cells; c++) mapped = mapped || (cells[c].n_out && cells[c].map_nout);
  if (mapped) { launch_resample_map(src, cells, n_cells, s); return; }   // no cell of the launch is mapped: the kernels and arguments below, as they always were
  LsnResampleCellsArgs P;
  LsnResampleWideCellsArgs Q;
  memset(&P, 0, sizeof(P));
  memset(&Q, 0, sizeof(Q));
  uint32_t n = 0, span = 0, nw = 0, span_w = 0;
  uint64_t runs = 0, runs_w = 0;
  for (uint32_t c = 0; c < n_cells; c++) {
    if (!cells[c].n_out) continue;
    if (cells[c].grp) {
      LsnResampleWideArgs& W = Q.c[nw++];
      runs_w = std::max(runs_w, resample_args(kernel, src, cells[c], W.a));
      W.grp = cells[c].grp; W.run = cells[c].run;
      span_w = std::max(span_w, cells[c].span);
    } else {
      runs = std::max(runs, resample_args(kernel, src, cells[c], P.c[n++]));
      span = std::max(span, cells[c].span);
    }
  }
  if (n) {
    const dim3 g((uint32_t)runs, src.nant, n);
    const size_t lds = (size_t)span * sizeof(float2);
    if (!rn) LSN_LAUNCH_FMT(k_resample_cells, , src.fmt, g, dim3(256), lds, s, P);
    else LSN_LAUNCH_FMT(k_resample_ring, , src.fmt, g, dim3(256), lds, s, P);
  }
  if (nw) {
    const dim3 g((uint32_t)runs_w, src.nant, nw);
    const size_t lds = (size_t)span_w * sizeof(float2);
    if (!rn) LSN_LAUNCH_FMT(k_resample_cells_wide, , src.fmt, g, dim3(256), lds, s, Q);
    else LSN_LAUNCH_FMT(k_resample_ring_wide, , src.fmt, g, dim3(256), lds, s, Q);
  }
}

// Strip-walk form of the separable 'same' convolution (rank-1 PSFs -- every sampled Gaussian -- whose non-zero taps fit a
// frame of 17 or of 33 taps per direction; the text below describes the 17-tap frame, the 33-tap frame is the same walk on
// 36 accumulator rows and two columns per lane).
//
// The tile kernel of sepconv.hip stages a (32 + halo) x (64 + halo) window in LDS, runs the row pass over ALL window
// rows (1.63 x the output rows) into a second LDS image, then the column pass: ~1000 vector instructions and ~200 KB of
// LDS traffic per 2048-pixel tile make it issue / LDS bound at 55-60 % of the HBM rate.  Here ONE WAVE owns a strip of
// 64 C columns (C = 2 or 4 per lane) and walks down R rows of it:
//   * per image row: the lanes multiply flux x exposure for their C columns, exchange the products through a
//     (64 C + 16)-float LDS row (one store, (16 + C) / 4 reads per lane), and run the 17-tap row pass on registers;
//   * the column pass is in SCATTER form: the finished row-pass value h[r] is added into the 17 outputs r - 8 .. r + 8
//     it contributes to, which live in 18 rotating accumulator slots of C registers per lane (the loop is unrolled over
//     the 18 rotation states so that every register index is static and the prefetch registers, period 2 or 3, rotate
//     with it); output row r - 8 is complete after row r and leaves the wave through the epilogue (Poisson pass, or
//     scale + accumulate for the adjoint).  At C = 4 the column pass runs on packed FMAs (two columns per instruction).
// No second LDS image, no block barriers, no halo rows recomputed inside a tile: 34 FMAs, 1 + (16 + C) / C LDS floats
// and one set of streaming loads per pixel; the only overhead is the 16 warm-up rows of a tile (R = 74: 22 % more row
// passes).  In the CHAINED form of the plain walk (walk_chain_kernel, walk_mixed_chain_kernel: blocks of up to four waves
// on vertically adjacent tiles; option JD_SEP_WALK_CHAIN) a wave takes the row-pass results of its last 16 rows from the
// LDS stash of the wave below it, which computes them anyway as its first 16: the warm-up rows then cost their loads and
// their column pass only.  It is the default where it was measured faster: the batched forward launch over both frames.
// Loads of row r + P are issued P steps ahead (registers), row taps live in SGPRs.  The launches follow their
// own instruction stream, not the memory system.
//
// Batched adjoint (the gradient of a joint step, sum over the datasets of E_d x corr(g_d, psf_d)): a block is one wave
// PER DATASET walking the same strip; finished rows go to an LDS exchange buffer in groups of 6, 3 or 2, and the waves
// add them in dataset order -- the additions of the per-dataset launches, bit for bit -- into the gradient image, which
// is read and written once.  Several flux components: walk_multi_kernel (forward, one wave per component) and the same
// adjoint over a grid of components x tiles with up to 16 waves per block.
//
// Units: walk_internal.h (frames, WalkArgs, the walk itself: walk_body and walk_kernel), this file (eligibility, frame
// selection, tiling, the plain walk and its chained and two-frame forms), walk_adjoint.hip (the exchange instantiations and
// both batched adjoints), walk_multi.hip (several flux components).  Every kernel instantiation is emitted by one unit.
//
// Until the commit "Split the strip walk into units; drop the fused step and dead switches" a fourth kernel family ran the
// WHOLE likelihood step of a one-component joint fit in one launch (walk_joint_kernel, option JD_SEP_JOINT = 1: a wave
// carried the forward and the adjoint convolution, the g images never existed, 13 instead of 29 B per (pixel, dataset)
// from HBM).  It agreed with the two launches bit for bit and lost to them: 201-205 us against 125 + 77.5 us at 2048^2 x 8,
// 134 against 63 + 49 us at four datasets (40 % more instructions for the halo, 150 registers); packed FMAs in both
// column passes, 13 % fewer vector instructions, took it from 201 to 197 us -- it is not the instruction count that
// bounds it.  DESIGN_LOG.md has the record.
#include "walk_internal.h"

namespace jd {

namespace {

// The chained plain walk: blocks of a.chain <= 4 waves; two waves per SIMD, whatever the block size
constexpr int CHAIN_MAX = 4;
template <int WKT, int C, int P, bool POISSON, bool IN_SCALE>
__global__ __launch_bounds__(64 * CHAIN_MAX, 2) void walk_chain_kernel(WalkArgs a) {
  walk_body<WKT, C, P, POISSON, IN_SCALE, 0, XW, true>(a, (int)blockIdx.x, a.strips, a.tiles_y, a.rows, POISSON ? 0 : a.order0);
}

// Batched forward launch over operators of both frames: the 17-tap datasets at C17 columns per lane, the 33-tap
// datasets behind them at two (every wave of the launch resident at once; the host sizes the two tilings so that the
// waves of both kinds take about as long).
template <int C17, int P>
__global__ __launch_bounds__(64) void walk_mixed_kernel(WalkArgs a) {
  if ((int)blockIdx.x < a.blocks17)  // (block-uniform)
    walk_body<17, C17, P, true, true, 0, XW>(a, (int)blockIdx.x, a.strips, a.tiles_y, a.rows, 0);
  else
    walk_body<33, 2, P, true, true, 0, XW>(a, (int)blockIdx.x - a.blocks17, a.strips33, a.tiles_y33, a.rows33, a.n17);
}

template <int C17, int P>
__global__ __launch_bounds__(64 * CHAIN_MAX, 2) void walk_mixed_chain_kernel(WalkArgs a) {
  if ((int)blockIdx.x < a.blocks17)  // (block-uniform)
    walk_body<17, C17, P, true, true, 0, XW, true>(a, (int)blockIdx.x, a.strips, a.tiles_y, a.rows, 0);
  else
    walk_body<33, 2, P, true, true, 0, XW, true>(a, (int)blockIdx.x - a.blocks17, a.strips33, a.tiles_y33, a.rows33, a.n17);
}

}  // namespace

// Do the walk kernels take a launch over n datasets of (H, W) pixels at all?  Option JD_SEP_WALK: 0 never, 1 whenever
// the operators allow (then independent of n: a batched step and the per-dataset calls it stands for choose alike and
// agree bit for bit), unset: where they are the faster kernels -- which depends on n, so that by default a batched step
// at a large size and its per-dataset form agree to fp32 rounding only.
bool walk_enabled(int H, int W, int n) {
  const int mode = opt_value(OPT_SEP_WALK, -1);
  if (mode == 0 || W % 4 != 0) return false;
  if (mode < 0 && (size_t)H * W * n < WALK_MIN_PIXELS) return false;
  return true;
}

// Do taps with the support `info` of a plan (kh, kw, oy, ox) fit a frame of WKf taps around position WHf, in both
// directions?  (Frame position of the stored row tap i: WHf + oy0 + i, of the stored column tap j: WHf + ox0 + j.)
static bool frame_fits(const SepOpInfo& info, int kh, int kw, int oy, int ox, int WHf, int WKf) {
  for (int adj = 0; adj < 2; ++adj) {
    const SepGeom g = sep_geom(kh, kw, oy, ox, adj != 0);
    if (WHf + g.oy0 + info.ulo[adj] < 0 || WHf + g.oy0 + info.uhi[adj] > WKf) return false;
    if (WHf + g.ox0 + info.vlo[adj] < 0 || WHf + g.ox0 + info.vhi[adj] > WKf) return false;
  }
  return true;
}

int walk_info_frame(const SepOpInfo& info, int kh, int kw, int oy, int ox) {
  if (info.rank != 1) return 0;
  if (frame_fits(info, kh, kw, oy, ox, Frame<17>::WH, Frame<17>::WK)) return 17;
  if (frame_fits(info, kh, kw, oy, ox, Frame<33>::WH, Frame<33>::WK)) return 33;
  return 0;
}

// The frame (17 or 33 taps) the walk kernels run a REGISTERED rank-1 operator of the plan geometry in, 0: none
int walk_operator_frame(const float* op, int kh, int kw, int oy, int ox) {
  SepOpInfo info;
  if (!sep_operator_info(op, &info)) return 0;
  return walk_info_frame(info, kh, kw, oy, ox);
}

// the widest support a plan of this geometry can hold (a full kh x kw PSF)
int plan_frame(int kh, int kw, int oy, int ox) {
  SepOpInfo full;
  full.rank = 1;
  for (int adj = 0; adj < 2; ++adj) {
    const SepGeom g = sep_geom(kh, kw, oy, ox, adj != 0);
    full.ulo[adj] = 0, full.uhi[adj] = kh, full.vlo[adj] = g.shiftx, full.vhi[adj] = g.shiftx + kw;
  }
  return walk_info_frame(full, kh, kw, oy, ox);
}

int device_cus() {
  static int n_cu = 0;
  if (!n_cu) {
    int dev = 0;
    hipDeviceProp_t prop;
    n_cu = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  return n_cu;
}

// (C, rows) of a launch over `n` datasets.  Measured inside the fit (tools/ab.py, MI355X): the launch is fastest with as
// many waves as are resident at once -- 8 per CU at C = 4 (218 registers: two per SIMD) -- and no second round: forward
// + Poisson launch of 2048^2 x 8 at C = 4 (after the packed column pass), rows 56 / 65 / 74 / 83 / 92 / 110 / 128 =
// 137 / 118 / 119 / 128 / 122 / 123 / 125 us (9.25 / 8 / 7 / 6.25 / 5.75 / 4.75 / 4 waves per CU); 4096^2 x 1 forward,
// rows 38 / 56 / 74 = 77 / 81 / 86 us (6.75 waves per CU at 38).  Rows = k WS - 2 WH: the walk advances in rounds of WS
// rows (18 k - 16 in the 17-tap frame, 36 k - 32 in the 33-tap frame, which always runs two columns per lane).
void walk_shape(int H, int W, int n, bool adjoint, int frame, int* C, int* rows) {
  const long want = (long)(7.25 * device_cus());
  auto waves = [&](int c, int r) { return walk_tile_count(H, W, c, r) * n; };
  const int ws = frame_ws(frame);
  if (frame == 33) {
    *C = 2, *rows = 2 * ws - 2 * Frame<33>::WH;
  } else {
    *C = waves(4, 38) >= want * 5 / 8 ? 4 : 2;
    *rows = 38;
  }
  while (*rows < 4096 && waves(*C, *rows) > want) *rows += ws;
  const int oc = opt_value(adjoint ? OPT_SEP_WALK_ADJ_COLS : OPT_SEP_WALK_COLS, 0);
  const int orows = opt_value(adjoint ? OPT_SEP_WALK_ADJ_ROWS : OPT_SEP_WALK_ROWS, 0);
  if ((oc == 2 || oc == 4) && frame != 33) *C = oc;
  if (orows >= 20 && orows <= 4096) *rows = orows;
}

// Chain length of a plain walk launch on tiles of `rows` rows: option JD_SEP_WALK_CHAIN (1-4; JD_SEP_WALK_ADJ_CHAIN, where
// set, for plain adjoints and the addend launch), else the launch's own default;
// 1 unless the tiles are k WS - 2 WH rows tall, k >= 2 (the heights walk_shape chooses: the hand-over then falls on the
// last 2 WH steps of a round behind the block barrier).
// Defaults, measured inside the fit on MI355X (tools/ab.py, profiles/walk_chain/README.md): the batched forward launch over
// both frames (2048^2, 6 + 2 datasets) 126.7 -> 119.5 us at chains of 4 (2: 130.6, 3: 155.5 -- three-wave blocks do not
// fill the eight wave slots of a CU); the addend launch, which runs beside the GMM screen kernel, +11 us per step at chains
// of 4 and no gain at 2 (a block needs its wave slots and up to 56 KB of LDS on ONE CU at once); forward launch and adjoint of one
// 4096^2 dataset (memory bound) 91.7 -> 93.0 and 46.9 -> 50.7 us.  A batched launch of one frame is unmeasured.
// The mixed launch takes its chains only where all of its blocks are resident at once (walk_conv_poisson_batch).
int walk_chain(int dflt, int frame, int rows, bool adjoint) {
  int L = opt_value(OPT_SEP_WALK_CHAIN, dflt);
  if (adjoint) L = opt_value(OPT_SEP_WALK_ADJ_CHAIN, L);  // (tuning: the adjoint-side launches apart from the forward ones)
  L = L < 1 ? 1 : L > CHAIN_MAX ? CHAIN_MAX : L;
  const int ws = frame_ws(frame), wh = frame_wh(frame);
  return (rows + 2 * wh) % ws == 0 && rows + 2 * wh >= 2 * ws ? L : 1;
}
// LDS of a chained block: L row buffers and L - 1 stashes of 2 WH rows (56 KB at L = 4 in both frames' widest form)
size_t chain_lds_bytes(int L, int frame, int C) {
  return (size_t)(L * 2 * 64 * C + (L - 1) * 2 * frame_wh(frame) * 64 * C) * sizeof(float);
}
// blocks per dataset of a tiling in chains of L: a multiple of 8 (the XCD-aware order)
int walk_blocks(int strips, int tiles_y, int L) { return (strips * ((tiles_y + L - 1) / L) + 7) / 8 * 8; }

// frame of one (dataset, component) entry of a batch: operator registered with rank 1 and a support that fits a frame,
// every image 16-byte aligned; 0: not a walk case
int dataset_frame(const SepBatchTable& t, int i, int d, int kh, int kw, int oy, int ox) {
  if (!(aligned16(t.scale[i]) && aligned16(t.g[i]) && aligned16(t.bkg[d]) && aligned16(t.cnt[d]))) return 0;
  return walk_operator_frame(t.op[i], kh, kw, oy, ox);
}

namespace {

// the plain walk of a.chain-wave blocks over n_grid datasets (no guard check, no profile scope: the callers')
template <bool POISSON, bool IN_SCALE>
void launch_plain(const WalkArgs& a, int frame, int C, int n_grid, hipStream_t stream) {
  const int L = a.chain > 1 ? a.chain : 1;
  const unsigned blocks = (unsigned)(walk_blocks(a.strips, a.tiles_y, L) * n_grid);
  const size_t lds = L > 1 ? chain_lds_bytes(L, frame, frame == 33 ? 2 : C) : 0;
  auto go = [&](void (*single)(WalkArgs), void (*chained)(WalkArgs)) {
    void (*kernel)(WalkArgs) = L > 1 ? chained : single;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * L), lds, stream, a);
  };
  constexpr int P = WALK_PREFETCH;
  if (frame == 33) go(walk_kernel<33, 2, P, POISSON, IN_SCALE, 0>, walk_chain_kernel<33, 2, P, POISSON, IN_SCALE>);
  else if (C == 4) go(walk_kernel<17, 4, P, POISSON, IN_SCALE, 0>, walk_chain_kernel<17, 4, P, POISSON, IN_SCALE>);
  else go(walk_kernel<17, 2, P, POISSON, IN_SCALE, 0>, walk_chain_kernel<17, 2, P, POISSON, IN_SCALE>);
}

template <bool POISSON, bool IN_SCALE>
int launch_walk(WalkArgs a, int frame, int C, int n_grid, hipStream_t stream) {
  int rc = sep_guard_check(&a.guard);
  if (rc) return rc;
  ProfScope prof(POISSON ? JD_KERNEL_POISSON_FUSED : JD_KERNEL_SEP_CONV, stream);
  launch_plain<POISSON, IN_SCALE>(a, frame, C, n_grid, stream);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace

void walk_plain_adjoint_launch(const void* walk_args, int frame, int C, int n_grid, hipStream_t stream) {
  launch_plain<false, false>(*static_cast<const WalkArgs*>(walk_args), frame, C, n_grid, stream);
}
int walk_plain_adjoint_checked(const void* walk_args, int frame, int C, int n_grid, hipStream_t stream) {
  return launch_walk<false, false>(*static_cast<const WalkArgs*>(walk_args), frame, C, n_grid, stream);
}

bool walk_takes_launch(int H, int W, int n_datasets, int kh, int kw, int oy, int ox) {
  return walk_enabled(H, W, n_datasets) && plan_frame(kh, kw, oy, ox) != 0;
}

// order <- the datasets with the 17-tap operators first (in dataset order), then the others; *n17 <- how many
void walk_batch_order(SepBatchTable& table, int n, int n_comp, int kh, int kw, int oy, int ox) {
  int k = 0;
  table.n17 = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int d = 0; d < n; ++d) {
      const bool is17 = n_comp != 1 || walk_operator_frame(table.op[d], kh, kw, oy, ox) != 33;
      if (is17 == (pass == 0)) table.order[k++] = d;
      if (is17 && pass == 0) ++table.n17;
    }
  for (; k < SEP_MAX_BATCH; ++k) table.order[k] = 0;
  table.frame33 = 0;
  for (int i = 0; i < n * n_comp && i < 64; ++i)
    if (walk_operator_frame(table.op[i], kh, kw, oy, ox) == 33) table.frame33 |= 1ull << i;
}

bool sep_batch_is_mixed(int n, int n_comp, const SepBatchTable& table, int H, int W, int kh, int kw, int oy, int ox) {
  // (the per-dataset calls a mixed batch falls back to decide with n = 1)
  if (n_comp > MULTI_MAX || !walk_enabled(H, W, n * n_comp)) return false;  // no dataset takes the walk kernels
  int yes = 0;
  for (int d = 0; d < n; ++d)
    for (int c = 0; c < n_comp; ++c) {
      const int f = dataset_frame(table, d * n_comp + c, d, kh, kw, oy, ox);
      yes += f != 0 ? 1 : 0;
    }
  return yes != 0 && yes != n * n_comp;
}

// A step over datasets of both frames, all of one frame in front of all of the other and at most SEP_ADDEND_MAX of the
// second: the first dataset of the second frame (walk_conv_adjoint_batch can leave the adjoints from there on in addend
// images).  n: no such split (one frame, interleaved frames, too many late datasets, not a walk case, option
// JD_SEP_ADJ_ADDENDS = 0).
int sep_addend_split(int n, const SepBatchTable& table, int H, int W, int kh, int kw, int oy, int ox) {
  if (opt_value(OPT_SEP_ADJ_ADDENDS, 1) == 0 || n < 2 || n > SEP_MAX_BATCH || !walk_enabled(H, W, n)) return n;
  int first = n, f0 = 0;
  for (int d = 0; d < n; ++d) {
    const int f = dataset_frame(table, d, d, kh, kw, oy, ox);
    if (!f) return n;
    if (d == 0) f0 = f;
    if (first == n && f != f0) first = d;
    if (first != n && f == f0) return n;  // (the first frame again: the dataset order is not frame order)
  }
  return n - first <= SEP_ADDEND_MAX ? first : n;
}

// out (+)= coef * out_scale * conv/corr_same(in * in_scale, psf)      [launch_sep_conv's contract]
int walk_conv(const float* in, const float* in_scale, const float* op, float* out, const float* out_scale, int H, int W,
              int kh, int kw, int oy, int ox, int adjoint, float coef, int accumulate, hipStream_t stream) {
  if (!walk_enabled(H, W, 1)) return JD_WALK_NOT_TAKEN;
  const int frame = walk_operator_frame(op, kh, kw, oy, ox);
  if (!frame) return JD_WALK_NOT_TAKEN;
  if (!aligned16(in) || !aligned16(in_scale) || !aligned16(out) || !aligned16(out_scale)) return JD_WALK_NOT_TAKEN;
  WalkArgs a{};
  a.in = in, a.in_scale = in_scale, a.op = op, a.out = out, a.out_scale = out_scale;
  a.H = H, a.W = W, a.coef = coef, a.accumulate = accumulate;
  walk_setup(a, kh, kw, oy, ox, adjoint);
  const int C = walk_plain_shape(a, 1, adjoint != 0, frame);
  return in_scale ? launch_walk<false, true>(a, frame, C, 1, stream) : launch_walk<false, false>(a, frame, C, 1, stream);
}

// launch_sep_conv_poisson's contract; *n_partials = partial sums written
int walk_conv_poisson(const float* in, const float* in_scale, const float* op, float* g_out, int H, int W, int kh, int kw,
                      int oy, int ox, const float* background, const float* counts, float* npred_out, double* partials,
                      float eps, float inv_n, int write_grad, int* n_partials, hipStream_t stream) {
  if (!walk_enabled(H, W, 1) || !in_scale) return JD_WALK_NOT_TAKEN;
  const int frame = walk_operator_frame(op, kh, kw, oy, ox);
  if (!frame) return JD_WALK_NOT_TAKEN;
  if (!aligned16(in) || !aligned16(in_scale) || !aligned16(g_out) || !aligned16(background) || !aligned16(counts) ||
      !aligned16(npred_out))
    return JD_WALK_NOT_TAKEN;
  WalkArgs a{};
  a.in = in, a.in_scale = in_scale, a.op = op, a.out = g_out;
  a.H = H, a.W = W, a.coef = 1.f;
  a.background = background, a.counts = counts, a.npred_out = npred_out, a.partials = partials;
  a.eps = eps, a.inv_n = inv_n, a.write_grad = write_grad;
  walk_setup(a, kh, kw, oy, ox, 0);
  const int C = walk_plain_shape(a, 1, false, frame);
  *n_partials = a.strips * a.tiles_y;
  return launch_walk<true, true>(a, frame, C, 1, stream);
}

// One flux component: all forward models + Poisson passes of a joint step in one launch (dataset-major grid, the
// datasets in table.order: 17-tap operators first); *n_partials = partial sums per dataset,
// partials[d * *n_partials + tile]
int walk_conv_poisson_batch(int n, const float* flux, const SepBatchTable& table, const SepBatchTable* table_dev, int H,
                            int W, int kh, int kw, int oy, int ox, double* partials, float eps, float inv_n,
                            int write_grad, int* n_partials, hipStream_t stream) {
  if (!walk_enabled(H, W, n) || !aligned16(flux)) return JD_WALK_NOT_TAKEN;
  int n17 = 0, n33 = 0;
  for (int d = 0; d < n; ++d) {
    const int f = dataset_frame(table, d, d, kh, kw, oy, ox);
    if (!f) return JD_WALK_NOT_TAKEN;
    (f == 17 ? n17 : n33)++;
  }
  if (n17 != table.n17) return fail(JD_ERR_INVALID, "walk_conv_poisson_batch: the table's dataset order is stale");
  WalkArgs a{};
  a.in = flux, a.H = H, a.W = W, a.coef = 1.f, a.partials = partials;
  a.eps = eps, a.inv_n = inv_n, a.write_grad = write_grad, a.n_batch = n, a.table = table_dev;
  walk_setup(a, kh, kw, oy, ox, 0);
  if (n17 == 0 || n33 == 0) {
    const int frame = n33 ? 33 : 17;
    const int C = walk_plain_shape(a, n, false, frame);
    *n_partials = a.strips * a.tiles_y;
    if (opt_is_set(OPT_SEP_INTERLEAVE)) a.ilv17 = n;
    return launch_walk<true, true>(a, frame, C, n, stream);
  }
  // Both frames in one launch, all waves resident at once.  A 17-tap wave at 4 columns per lane issues ~226 vector
  // instructions per row of 256 pixels, a 33-tap wave at 2 columns ~COST33 per row of 128; the two tilings are chosen so
  // that tile time (cost per row x (rows + warm-up rows)) is about equal and the waves fill the chip once.  Measured
  // inside the fit (tools/ab.py, 2048^2, 6 + 2 datasets): COST33 = 150 / 190 / 230 / 260 / 280 -> 139.5 / 124.4-126.9 /
  // 123.0-124.9 / 122.8-124.4 / 125.0 us: 230 it is.
  const double cost17_4 = 226.0, cost17_2 = 150.0, cost33 = 230.0;
  const long want = (long)(7.25 * device_cus());
  auto tiles = [&](int c, int r) { return walk_tile_count(H, W, c, r); };
  int C = tiles(4, 38) * n17 + tiles(2, 40) * n33 >= want * 5 / 8 ? 4 : 2;
  const int oc = opt_value(OPT_SEP_WALK_COLS, 0);
  if (oc == 2 || oc == 4) C = oc;
  const double cost17 = C == 4 ? cost17_4 : cost17_2;
  int rows = 38, rows33 = 40;
  for (int r17 = 38; r17 < 4096; r17 += Frame<17>::WS) {
    // the 33-tap tile height (36 k - 32) whose tile time is nearest that of the 17-tap tile
    const double t17 = cost17 * (r17 + 2 * Frame<17>::WH);
    int k = (int)std::lround(t17 / cost33 / Frame<33>::WS);  // (rows + 2 WH = k WS)
    if (k < 2) k = 2;
    const int r33 = k * Frame<33>::WS - 2 * Frame<33>::WH;
    rows = r17, rows33 = r33;
    if (tiles(C, r17) * n17 + tiles(2, r33) * n33 <= want) break;
  }
  const int orows = opt_value(OPT_SEP_WALK_ROWS, 0), orows33 = opt_value(OPT_SEP_WALK_ROWS33, 0);
  if (orows >= 20 && orows <= 4096) rows = orows;
  if (orows33 >= 20 && orows33 <= 4096) rows33 = orows33;
  walk_tiles(a, C, rows);
  a.rows33 = rows33, a.strips33 = (W + 127) / 128, a.tiles_y33 = (H + rows33 - 1) / rows33;
  const int t17 = a.strips * a.tiles_y, t33 = a.strips33 * a.tiles_y33;
  a.n17 = n17;
  if (opt_is_set(OPT_SEP_INTERLEAVE)) a.ilv17 = n17, a.ilv33 = n33;
  // (one block size per launch: both frames' tiles chained alike, or -- a tiling of either no taller than a round -- not at all)
  int L = std::min(walk_chain(CHAIN_MIXED, 17, rows), walk_chain(CHAIN_MIXED, 33, rows33));
  // Every block of the launch must be resident at once, as every wave is with one wave per block: the tilings above are
  // sized in single waves, but a chain is rounded up to whole blocks (per strip, and to 8 blocks per dataset), and a CU
  // holds only as many blocks of L waves as its 8 wave slots and its 160 KB of LDS allow -- two at L = 4.  A launch with
  // more blocks than that runs a second round of them (measured with three-wave blocks, which do not fill the slots
  // either: 155.5 against 126.7 us), so the DEFAULT chain length is taken only where the blocks fit, else 1 (chains of 2
  // and 3 were measured slower than single waves where they do fit).  An option set by hand is taken as it is.
  const size_t lds = L > 1 ? std::max(chain_lds_bytes(L, 17, C), chain_lds_bytes(L, 33, 2)) : 0;  // (L only ever falls to 1 below)
  if (L > 1 && !opt_is_set(OPT_SEP_WALK_CHAIN)) {
    const long per_cu = std::min<long>(8 / L, (long)(160 * 1024 / lds));
    const long blocks = (long)walk_blocks(a.strips, a.tiles_y, L) * n17 + (long)walk_blocks(a.strips33, a.tiles_y33, L) * n33;
    if (blocks > per_cu * device_cus()) L = 1;
  }
  a.chain = L;
  a.blocks17 = walk_blocks(a.strips, a.tiles_y, L) * n17;
  a.part_stride = t17 > t33 ? t17 : t33;
  *n_partials = a.part_stride;
  int rc = sep_guard_check(&a.guard);
  if (rc) return rc;
  const unsigned blocks = (unsigned)(a.blocks17 + walk_blocks(a.strips33, a.tiles_y33, L) * n33);
  ProfScope prof(JD_KERNEL_POISSON_FUSED, stream);
  void (*kernel)(WalkArgs) = L > 1 ? (C == 4 ? walk_mixed_chain_kernel<4, WALK_PREFETCH> : walk_mixed_chain_kernel<2, WALK_PREFETCH>)
                                   : (C == 4 ? walk_mixed_kernel<4, WALK_PREFETCH> : walk_mixed_kernel<2, WALK_PREFETCH>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * L), L > 1 ? lds : 0, stream, a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace jd

// Strip-walk convolution (walkconv.hip has the method): the batched adjoints -- the exchange instantiations of
// walk_kernel (XG > 0: one wave per dataset, finished rows added in dataset order through LDS) and their two launchers.
#include "walk_internal.h"

namespace jd {

namespace {

constexpr int XW2 = 16;  // waves per block of the adjoint over all components (walk_conv_adjoint_batch_all)

// Block shape of an exchange launch of `n` waves (= datasets) in `frame`.  6-8 datasets: 4 columns per lane (1 KB per row
// and stream), exchange groups of 6 rows: 112 KB of LDS, ONE block of 6-8 waves per CU; fewer datasets: 2 columns per lane,
// as many blocks per CU as LDS (exchange buffer) and registers (112-127: 4 waves per SIMD) allow.  Rows per tile: a
// multiple of every exchange group size, the smallest that leaves all blocks resident at once.  Measured inside the fit
// at 2048^2 x 8 (tools/ab.py): C = 4, rows 36 / 66 / 72 / 84 = 98 / 77.5 / 85 / 89 us (66 rows: 8 strips x 32 tiles = one
// block for every CU); C = 2 (two blocks per CU), rows 54 / 72 / 90 = 111 / 85 / 97 us.  The 33-tap frame: two columns per
// lane, two waves per SIMD.  big: up to XW2 waves; n_comp: components the grid covers; orows: the caller's tile height option.
struct ExchangeShape {
  int xg, C, waves, lds, rows;  // rows per group, columns per lane, waves the kernel is compiled for (XWT), LDS bytes
};
ExchangeShape exchange_shape(int H, int W, int frame, int n, int n_comp, bool big, int orows) {
  ExchangeShape s;
  s.xg = n >= 6 ? 6 : n >= 3 ? 3 : 2;
  const bool wide = frame == 17 && !big && n >= 6 && opt_value(OPT_SEP_WALK_ADJ_COLS, 4) != 2;
  s.C = wide ? 4 : 2;
  s.waves = big ? XW2 : XW;
  s.lds = (2 * s.xg * s.waves * 64 * s.C + s.waves * 128 * s.C) * 4;  // exchange buffer + row buffers
  int per_cu = 160 * 1024 / s.lds;
  // (204 registers at C = 4 and in the 33-tap frame: 2 waves per SIMD; 112-127 at C = 2 in the 17-tap frame: 4)
  const int by_regs = (wide || frame == 33 ? 8 : 16) / n;
  if (per_cu > by_regs) per_cu = by_regs;
  if (per_cu < 1) per_cu = 1;
  const long slots = (long)device_cus() * per_cu * (per_cu > 1 ? 15 : 16) / 16;
  s.rows = 36;
  while (s.rows < 4096 && walk_tile_count(H, W, s.C, s.rows) * n_comp > slots) s.rows += 6;
  if (orows >= 18) s.rows = orows;
  s.rows = (s.rows + 5) / 6 * 6;
  return s;
}

// the exchange instantiation of (frame, C, xg, big) on blocks of `waves` waves
void launch_exchange(const WalkArgs& a, int frame, const ExchangeShape& s, unsigned blocks, int waves, hipStream_t stream) {
  auto go = [&](void (*kernel)(WalkArgs)) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * waves), 0, stream, a); };
  constexpr int P = WALK_PREFETCH;
  if (s.waves == XW2) go(walk_kernel<17, 2, P, false, false, 6, XW2>);
  else if (frame == 33 && s.xg == 6) go(walk_kernel<33, 2, P, false, false, 6>);
  else if (frame == 33 && s.xg == 3) go(walk_kernel<33, 2, P, false, false, 3>);
  else if (frame == 33) go(walk_kernel<33, 2, P, false, false, 2>);
  else if (s.C == 4) go(walk_kernel<17, 4, WALK_PREFETCH_ADJ, false, false, 6>);
  else if (s.xg == 6) go(walk_kernel<17, 2, P, false, false, 6>);
  else if (s.xg == 3) go(walk_kernel<17, 2, P, false, false, 3>);
  else go(walk_kernel<17, 2, P, false, false, 2>);
}

// the loss fold of an exchange launch (blocks d < n: dataset d's loss) needs 256 threads and a block per dataset
bool arm_loss_fold(WalkArgs& a, const double* fin_partials, double fin_scale, int fin_count, int n, int waves, unsigned blocks) {
  if (!fin_partials || waves < 4 || (int)blocks < n) return false;
  a.fin_partials = fin_partials, a.fin_scale = fin_scale, a.fin_count = fin_count, a.fin_n = n;
  return true;
}

}  // namespace

// grad (+)= coef * sum_d scale[d] * corr_same(g[d], psf_d), the datasets added in order: one wave per dataset, up to 8
// datasets per launch, later chunks accumulate (the same additions in the same order).  Datasets whose operators walk
// in different frames go to different launches: the batch is cut into runs of consecutive datasets of one frame (the
// benchmark's 6 + 2), so the order of the additions stays the dataset order.  With fin_partials, blocks d < n of the
// first launch also turn the fin_count partial sums of dataset d into its loss (*fin_done <- 1)
int walk_conv_adjoint_batch(int n, int n_comp, int comp, const SepBatchTable& table, const SepBatchTable* table_dev,
                            float* grad, int H, int W, int kh, int kw, int oy, int ox, float coef, int accumulate,
                            hipStream_t stream, const double* fin_partials, double fin_scale, int fin_count, int* fin_done,
                            int addend_first, hipStream_t stream2, const hipEvent_t* fork_join) {
  *fin_done = 0;
  if (!walk_enabled(H, W, n * n_comp) || !aligned16(grad)) return JD_WALK_NOT_TAKEN;
  int frames[SEP_MAX_BATCH];
  for (int d = 0; d < n; ++d)
    for (int c = 0; c < n_comp; ++c) {  // (all components: the forward launch of the step must have been a walk launch too)
      const int f = dataset_frame(table, d * n_comp + c, d, kh, kw, oy, ox);
      if (!f) return JD_WALK_NOT_TAKEN;
      if (c == comp) frames[d] = f;
    }
  WalkArgs a{};
  a.out = grad, a.H = H, a.W = W, a.coef = coef, a.table = table_dev, a.n_comp = n_comp, a.comp = comp;
  walk_setup(a, kh, kw, oy, ox, 1);
  int rc = sep_guard_check(&a.guard);
  if (rc) return rc;
  // The adjoints of the datasets [addend_first, n) (the caller's sep_addend_split: one frame, at most SEP_ADDEND_MAX) go to
  // images of their own, table.addend[d] = (coef * corr(g_d, psf_d)) * E_d -- the value the exchange path below adds into
  // the gradient image -- by the plain walk: one wave per (dataset, tile), no exchange, no barrier, and no access to the
  // gradient image, so the launch depends on the forward launch alone and runs on stream2 BESIDE the launch(es) of the
  // datasets in front of it (fork behind the forward launch, join before this call returns: a captured epoch sees a
  // closed branch).  Whoever consumes the gradient adds the addends in dataset order (jd_adam.h): the same additions.
  int n_main = n;
  hipEvent_t join = nullptr;
  if (addend_first > 0 && addend_first < n) {
    const int m = n - addend_first, frame = frames[addend_first];
    if (n_comp != 1 || m > SEP_ADDEND_MAX || !table_dev) return fail(JD_ERR_INVALID, "walk_conv_adjoint_batch: not an addend split");
    for (int d = addend_first; d < n; ++d)
      if (frames[d] != frame || !table.addend[d] || !aligned16(table.addend[d]))
        return fail(JD_ERR_INVALID, "walk_conv_adjoint_batch: not an addend split");
    const bool beside = stream2 && stream2 != stream;
    if (beside && !(fork_join && fork_join[0] && fork_join[1]))
      return fail(JD_ERR_INVALID, "walk_conv_adjoint_batch: a second stream needs the caller's fork and join events");
    const hipStream_t s2 = beside ? stream2 : stream;
    WalkArgs b = a;
    b.out = nullptr, b.n_batch = m, b.accumulate = 0;
    b.order0 = frame == 33 ? table.n17 : 0;  // (table.order: the 17-tap datasets, then the 33-tap ones, in dataset order)
    // Beside the main launch the tiles are sized for HALF of the wave slots walk_shape fills (taller tiles: fewer waves, and
    // fewer warm-up rows -- 32 per tile in the 33-tap frame).  Measured inside the fit (tools/ab.py, 2048^2, 6 + 2 datasets,
    // accumulating launches 591.6 us per step): 33-tap tiles of 40 / 76 / 112 / 148 / 220 rows = 579.0 / 574.3 / 577.6 /
    // 576.8 / 589.4 us (1664 / 864 / 608 / 448 / 320 waves beside the 1344 of the 17-tap launch; 40 is walk_shape's own
    // choice, 76 this rule's) -- profiles/adjoint_addends/sweep_rows33.txt.  One sweep at one shape (33-tap, two late
    // datasets): for a late 17-tap frame and for other sizes the rule is unmeasured.
    const int orows1 = opt_value(frame == 33 ? OPT_SEP_WALK_ADJ_ROWS33 : OPT_SEP_WALK_ADJ_ROWS, 0);
    // (tuning: the adjoint tile height option of the launch's frame)
    const int C1 = walk_plain_shape(b, m, true, frame, beside ? (long)(7.25 * device_cus()) / 2 : 0,
                                    orows1 >= 20 && orows1 <= 4096 ? orows1 : 0);
    if (beside) {
      JD_HIP(hipEventRecord(fork_join[0], stream));
      JD_HIP(hipStreamWaitEvent(stream2, fork_join[0], 0));
    }
    rc = walk_plain_adjoint_checked(&b, frame, C1, m, s2);
    if (beside) {
      // (from here on the branch is joined whatever fails: a capture is never left with an open branch)
      join = fork_join[1];
      // (a record that fails leaves nothing to join with: the error goes to the caller, whose capture, if any, is lost)
      const hipError_t e = hipEventRecord(join, s2);
      if (e != hipSuccess) return rc ? rc : fail(JD_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
    }
    if (rc) {
      if (join) (void)hipStreamWaitEvent(stream, join, 0);
      return rc;
    }
    n_main = addend_first;
  }
  // (the main stream goes on behind the addend launch however this function is left: no branch of a capture stays open)
  struct JoinOnExit {
    hipStream_t stream;
    hipEvent_t event;
    ~JoinOnExit() {
      if (event) (void)hipStreamWaitEvent(stream, event, 0);
    }
  } join_on_exit{stream, join};
  for (int d0 = 0; d0 < n_main;) {
    const int frame = frames[d0];
    int m = 1;
    while (d0 + m < n_main && m < XW && frames[d0 + m] == frame) ++m;  // datasets (= waves) of this launch: its block shape follows
    const int orows = opt_value(frame == 33 ? OPT_SEP_WALK_ADJ_ROWS33 : OPT_SEP_WALK_ADJ_ROWS, 0);
    a.d_base = d0, a.n_batch = m, a.accumulate = d0 == 0 ? accumulate : 1;
    a.fin_partials = nullptr;
    if (m == 1) {  // a single dataset: the plain walk (same arithmetic: out (+)= (coef * corr) * scale)
      WalkArgs b = a;
      const int slot = d0 * n_comp + comp;
      b.n_batch = 0, b.table = nullptr, b.in = table.g[slot], b.op = table.op[slot], b.out_scale = table.scale[slot];
      const int C1 = walk_plain_shape(b, 1, true, frame, 0, frame == 33 && orows >= 18 ? orows : 0);
      ProfScope prof(JD_KERNEL_SEP_CONV, stream);
      walk_plain_adjoint_launch(&b, frame, C1, 1, stream);
    } else {
      const ExchangeShape s = exchange_shape(H, W, frame, m, 1, false, orows);
      walk_tiles(a, s.C, s.rows);
      const unsigned blocks = (unsigned)walk_blocks(a.strips, a.tiles_y, 1);
      if (arm_loss_fold(a, d0 == 0 ? fin_partials : nullptr, fin_scale, fin_count, n, m, blocks)) *fin_done = 1;
      ProfScope prof(JD_KERNEL_SEP_CONV, stream);
      launch_exchange(a, frame, s, blocks, m, stream);
    }
    JD_LAUNCH_CHECK();
    d0 += m;
  }
  return JD_OK;
}

// The same sum for ALL flux components of up to 16 datasets in ONE launch: grads[c] (+)= coef * sum_d scale[d, c] *
// corr_same(g[d, c], psf_(d, c)).  The grid is n_comp x tiles, a block is one wave per dataset (up to 16: a full 1024
// threads, two columns per lane so that 128 registers do), the datasets are added in order as above -- the same bits as
// the per-component launches in chunks of 8, which at the benchmark's two-component case (1024^2 x 16 x 2) meant four
// launches that each filled under half of the chip.  Option JD_SEP_WALK_ADJ_ALL = 0: never.
int walk_conv_adjoint_batch_all(int n, int n_comp, const SepBatchTable& table, const SepBatchTable* table_dev,
                                float* const* grads, int H, int W, int kh, int kw, int oy, int ox, float coef, int accumulate,
                                hipStream_t stream, const double* fin_partials, double fin_scale, int fin_count,
                                int* fin_done) {
  static_assert(MULTI_MAX <= 4, "WalkArgs::out_comp");
  *fin_done = 0;
  if (opt_value(OPT_SEP_WALK_ADJ_ALL, 1) == 0) return JD_WALK_NOT_TAKEN;
  if (n < 2 || n > XW2 || n_comp < 1 || n_comp > MULTI_MAX || (n <= XW && n_comp < 2) || !table_dev) return JD_WALK_NOT_TAKEN;
  // One component, 9-16 datasets: two launches of the 4-column kernel are the faster form where they fill the chip
  // (2048^2 x 16: 2 x 75.7 us against 163 us), this one where even 36-row tiles leave CUs without a block (1024^2 x
  // 16: 60 us against 2 x 49 us).  Two components at 2048^2 x 16: 296 us against 4 x 78 us.
  if (n_comp == 1 && walk_tile_count(H, W, 4, 36) >= device_cus()) return JD_WALK_NOT_TAKEN;
  WalkArgs a{};
  for (int c = 0; c < n_comp; ++c) {
    if (!aligned16(grads[c])) return JD_WALK_NOT_TAKEN;
    a.out_comp[c] = grads[c];
  }
  if (!walk_enabled(H, W, n * n_comp)) return JD_WALK_NOT_TAKEN;
  for (int d = 0; d < n; ++d)
    for (int c = 0; c < n_comp; ++c)  // (one launch = one frame: the 17-tap one)
      if (dataset_frame(table, d * n_comp + c, d, kh, kw, oy, ox) != 17) return JD_WALK_NOT_TAKEN;
  a.out = grads[0], a.H = H, a.W = W, a.coef = coef, a.table = table_dev, a.n_comp = n_comp, a.comp = 0;
  walk_setup(a, kh, kw, oy, ox, 1);
  int rc = sep_guard_check(&a.guard);
  if (rc) return rc;
  const ExchangeShape s = exchange_shape(H, W, 17, n, n_comp, n > XW, opt_value(OPT_SEP_WALK_ADJ_ROWS, 0));
  walk_tiles(a, s.C, s.rows);
  a.comp_blocks = walk_blocks(a.strips, a.tiles_y, 1);
  const unsigned blocks = (unsigned)a.comp_blocks * n_comp;
  a.d_base = 0, a.n_batch = n, a.accumulate = accumulate;
  if (arm_loss_fold(a, fin_partials, fin_scale, fin_count, n, n, blocks)) *fin_done = 1;
  ProfScope prof(JD_KERNEL_SEP_CONV, stream);
  launch_exchange(a, 17, s, blocks, n, stream);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace jd

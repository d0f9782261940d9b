// What the units of the strip-walk convolution share (walkconv.hip: the method, eligibility, tiling, the plain walk;
// walk_adjoint.hip: the batched adjoints; walk_multi.hip: several flux components): the frames and constants, the argument
// block, the walk itself (walk_body) with its kernel template, and the host helpers one unit calls in another.
// WalkArgs and the device code stay in the unnamed namespace -- the kernels' symbol names carry it -- so the host helpers
// that take a WalkArgs are inline here and the others are plain functions of walkconv.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>

#include "jd_common.h"
#include "kernels.h"

namespace jd {

namespace {

// The walk's FRAME: WK taps per direction, out[y] = sum_t tu[t] h[y - WH + t], and WS accumulator slots (the rotation
// period of the unrolled walk: > WK, and a multiple of every prefetch depth and exchange group size).  Two frames are
// compiled: 17 taps (PSFs up to 17 x 17, the common case) and 33 taps (up to 33 x 33; twice the arithmetic per pixel, two
// columns per lane so that its 36 accumulator rows fit the register file at two waves per SIMD).  Which frame an
// operator takes follows from the support of ITS taps (SepOpInfo), not from the plan's (kh, kw): datasets whose PSFs
// were embedded in a common larger array walk in the frame their own PSF needs.
template <int WKT> struct Frame;
template <> struct Frame<17> { static constexpr int WK = 17, WH = 8, WS = 18; };
template <> struct Frame<33> { static constexpr int WK = 33, WH = 16, WS = 36; };
// (a frame's WS / WH by value, for the host's tiling rules)
constexpr int frame_ws(int frame) { return frame == 33 ? Frame<33>::WS : Frame<17>::WS; }
constexpr int frame_wh(int frame) { return frame == 33 ? Frame<33>::WH : Frame<17>::WH; }
constexpr int XG_MAX = 6;  // rows per exchange group of the batched adjoint: 2, 3 or 6 (a divisor of WS, <= waves)
constexpr int XW = 8;   // waves (= datasets) per block of the batched adjoint
constexpr int MULTI_MAX = 4;  // flux components (= waves per block) of walk_multi_kernel; WalkArgs::out_comp
#ifndef JD_WALK_PREFETCH
#define JD_WALK_PREFETCH 2
#endif
constexpr int WALK_PREFETCH = JD_WALK_PREFETCH;  // rows the streaming loads run ahead of the arithmetic
// the batched adjoint on 4 columns per lane has one block of 8 waves per CU: its 32 KB in flight per CU at two rows
// ahead are the latency-bandwidth product of its 3.9 TB/s; three rows ahead: 80 -> 75 us in the fit (the forward launch
// loses 3 % with the extra registers: it stays at two)
constexpr int WALK_PREFETCH_ADJ = 3;
// Launches below this many (pixel, dataset) pairs stay with the tile kernel, which has four times the waves for the
// same image: measured on MI355X (tools/walk_check.py) forward + adjoint of one 2048^2 dataset 38.9 us (tile) against
// 51.8 (walk), of two 65 / 77, of four 129 / 112, of eight 282 / 199, of one 4096^2 dataset 138 / 118
constexpr size_t WALK_MIN_PIXELS = (size_t)1 << 24;

template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

template <int C> struct Vec;
template <> struct Vec<2> { typedef float T __attribute__((ext_vector_type(2))); };
template <> struct Vec<4> { typedef float T __attribute__((ext_vector_type(4))); };

struct WalkArgs {
  const float* in;         // forward: flux; plain / adjoint: the image to convolve
  const float* in_scale;   // forward: exposure
  const float* op;         // operator buffer of sepconv.hip
  float* out;              // POISSON: g = d loss / d conv; plain: the result (+= when accumulate)
  const float* out_scale;  // plain: nullable
  const float* background;
  const float* counts;
  float* npred_out;  // nullable
  double* partials;  // POISSON: one per (dataset, tile)
  int H, W, strips, tiles_y, rows;
  int taps_u, taps_v;          // op offsets of the first row tap / first column tap of this direction
  int kh, kw, oy0, ox0;        // the plan's PSF size; image offset of its first stored tap (frame position WH + oy0)
  // batched forward launch over operators of BOTH frames: blocks < blocks17 walk the 17-tap datasets
  // table->order[0 .. n17) with the tiling above, the others the 33-tap datasets table->order[n17 ..) with this one
  int blocks17, n17;
  int ilv17, ilv33;            // > 0 (tuning, JD_SEP_INTERLEAVE): the ilv datasets of a frame are neighbours in the launch order
  int strips33, tiles_y33, rows33;
  int part_stride;             // POISSON: partial sums per dataset in `partials` (>= tiles of either tiling; the rest zeroed)
  float coef;
  int accumulate;
  float eps, inv_n;
  int write_grad;
  int n_batch;                 // > 0: per-dataset pointers come from `table`
  const SepBatchTable* table;
  int d_base;                  // batched adjoint: first dataset of this launch (wave w = dataset d_base + w)
  int order0;                  // plain launch over several datasets (their adjoints into table->addend[d]): position of its
                               // first dataset in table->order
  int n_comp, comp;            // batched adjoint: components per dataset and the one of this launch (table entry d * n_comp + comp)
  const double* fin_partials;  // batched adjoint: blocks < fin_n finalise the losses of the forward launch
  double fin_scale;
  int fin_count, fin_n;
  int* guard;                  // host-mapped: set when an operator is not rank 1
  int comp_blocks;             // batched adjoint over ALL components: blocks per component (0: component `comp` only)
  int chain;                   // chained plain walk: waves (= vertically adjacent tiles of one strip) per block, 2-4
  float* out_comp[4];          //   and their gradient images
};

__device__ __forceinline__ void wave_lds_fence() {
  // LDS operations of one wave execute in order; this only keeps the COMPILER from moving them across
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// acc (+)= tap * h on packed fp32 (two pixels per instruction), the tap being the low (SEL = 0) or high (SEL = 1) half
// of a register pair broadcast to both elements through the operand-select bits -- hipcc has no pattern for that and
// otherwise spends a register pair per tap.  The same fused multiply-add (or plain product) per element as fmaf / *.
typedef float v2f __attribute__((ext_vector_type(2)));
template <int SEL>
__device__ __forceinline__ v2f pk_fma_tap(v2f taps, v2f h, v2f acc) {
  if constexpr (SEL == 0)
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(taps), "v"(h));
  else
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(taps), "v"(h));
  return acc;
}
template <int SEL>
__device__ __forceinline__ v2f pk_mul_tap(v2f taps, v2f h) {
  v2f r;
  if constexpr (SEL == 0)
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(taps), "v"(h));
  else
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(taps), "v"(h));
  return r;
}

// XG > 0: the batched adjoint (one wave per dataset -- at most XWT of them --, rows exchanged in groups of XG, wave
// w < XG adds up row w of a group); with a.comp_blocks > 0 the grid covers all flux components, comp_blocks blocks each.
// `bid`: the block's index within the blocks of its frame; (strips, tiles_y, rows): their tiling; `slot0`: position of
// the frame's first dataset in table->order (batched forward launches).
// CH: the CHAINED plain walk (XG == 0 only).  A block is a.chain waves that own vertically adjacent tiles of one strip of
// one dataset.  The first 2 WH rows a tile walks are the last 2 WH rows of the tile above it: every wave but the first
// of its chain stashes the row-pass results h of those rows in LDS as it computes them (2 WH rows of 64 C floats), one
// block barrier sits behind the first round of WS steps (WS > 2 WH: the stash is complete there; the host only chains
// tiles of k WS - 2 WH rows, k >= 2: their last 2 WH steps are the steps WS - 2 WH .. WS - 1 of a LATER round -- static
// places of the unrolled loop, chosen by one scalar flag per round), and a wave with a lower neighbour takes h of its last
// 2 WH rows from that neighbour's stash -- one LDS read per row instead of product, exchange and row pass.  The value is
// the one the wave would have computed (same loads, masks and arithmetic): the results are the same bits.  The streaming
// loads of the handed-over rows stay (every step issues the same loads: the compiler goes on counting them exactly).
template <int WKT, int C, int P, bool POISSON, bool IN_SCALE, int XG, int XWT, bool CH = false>
__device__ __forceinline__ void walk_body(const WalkArgs& a, int bid, const int strips, const int tiles_y, const int rows,
                                          const int slot0) {
#pragma clang fp contract(off)  // every fused multiply-add below is an explicit fmaf: batched and per-dataset paths round alike
  constexpr int WK = Frame<WKT>::WK, WH = Frame<WKT>::WH, WS = Frame<WKT>::WS;
  constexpr bool XCHG = XG > 0;
  static_assert(!XCHG || (WS % XG == 0 && XG <= XG_MAX), "the exchange group must divide the rotation period");
  static_assert(!(CH && XCHG), "the chained walk is the plain walk");
  static_assert(WS > 2 * WH, "the stash must be complete behind the first round");
  typedef typename Vec<C>::T vC;
  constexpr int NX = 2 * WH / C;       // lanes that also load the right-hand halo piece
  constexpr int NWIN = 2 * WH + C;     // window floats per lane
  static_assert(64 * C + C * 64 <= 2 * 64 * C && NX <= 64, "row buffer");
  __shared__ __attribute__((aligned(16))) float rowbuf[XCHG ? XWT : 1][2 * 64 * C];  // 64 C + 2 WH floats used, the rest is a dump
  __shared__ __attribute__((aligned(16))) float xbuf[XCHG ? 2 * XG * XWT * 64 * C : 4];
  // CH (dynamic, sized by the host): a.chain row buffers, then the stashes of the waves 1 .. a.chain - 1
  extern __shared__ __attribute__((aligned(16))) float chain_lds[];
  vC oprev;  // XCHG: the row of the gradient image this wave adds a group's row to, requested at the group's start
  __shared__ double fin_red[4];

  const int lane = threadIdx.x & 63;
  // (CH: scalar, so that everything derived from the wave's tile stays in SGPRs as it does with one wave per block)
  const int wv = XCHG ? (int)(threadIdx.x >> 6) : CH ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  const int nb = XCHG ? (int)(blockDim.x >> 6) : 1;

  if (XCHG && a.fin_partials && (int)blockIdx.x < a.fin_n) {  // (block-uniform; the host asks only with >= 256 threads)
    // finalize_rows_kernel's summation order: 256 strided threads, wave butterflies, the four wave sums in order
    if (threadIdx.x < 256) {
      const double* row = a.fin_partials + (size_t)blockIdx.x * a.fin_count;
      double s = 0.0;
      for (int i = threadIdx.x; i < a.fin_count; i += 256) s += row[i];
      s = wave_sum(s);
      if (lane == 0) fin_red[wv] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double total = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) total += fin_red[i];
      a.table->loss_out[blockIdx.x][0] = (float)(a.fin_scale * total + (double)a.table->loss_offset[blockIdx.x]);
    }
  }

  // consecutive tiles of one XCD (blockIdx % 8) are vertical neighbours in a strip: their halo rows hit in that L2
  // (CH: the same order in units of chains, chain k of a strip being its tiles k L .. k L + L - 1)
  const int n_tiles = strips * tiles_y;
  const int L = CH ? a.chain : 1;
  const int chains_y = CH ? (tiles_y + L - 1) / L : tiles_y;
  const int n_units = CH ? strips * chains_y : n_tiles;
  const int per_xcd = (n_units + 7) / 8;
  int comp = a.comp;
  if (XCHG && a.comp_blocks) comp = bid / a.comp_blocks, bid -= comp * a.comp_blocks;  // (comp_blocks: a multiple of 8)
  const int q = bid / 8;
  // batched forward launch: dataset-major, the datasets of this frame in the table's order
  // (JD_SEP_INTERLEAVE: tile-major instead -- the waves of one tile's datasets start together and read the flux rows they
  // share within a row or two of each other)
  const int ilv = !XCHG && a.n_batch > 0 ? (slot0 ? a.ilv33 : a.ilv17) : 0;
  const int dsel = (!XCHG && a.n_batch > 0) ? a.table->order[slot0 + (ilv ? q % ilv : q / per_xcd)] : 0;
  const int unit = (bid % 8) * per_xcd + (ilv ? q / ilv : q % per_xcd);
  if (unit >= n_units) return;  // (block-uniform)
  const int sx = unit / chains_y, ty = CH ? (unit - sx * chains_y) * L + wv : unit - sx * tiles_y;
  const int tile = CH ? sx * tiles_y + ty : unit;
  if constexpr (CH) {
    if (ty >= tiles_y) {  // (wave-uniform) a chain that ends at the image's last tile: no wave leaves before the barrier
      __syncthreads();
      return;
    }
  }

  // (global address space stated: pointers that come out of the table are generic to the compiler, and generic loads are
  // `flat_` instructions, which complete out of order and force a full s_waitcnt at every step)
  typedef const float __attribute__((address_space(1)))* gcp;
  typedef float __attribute__((address_space(1)))* gp;
  typedef const vC __attribute__((address_space(1)))* gcv;
  typedef vC __attribute__((address_space(1)))* gv;
  const bool batch = a.n_batch > 0;
  const int d = XCHG ? a.d_base + wv : dsel;
  const int slot = XCHG ? d * a.n_comp + comp : d;  // (a batched forward launch of this kernel has one component)
  const gcp in = (gcp)(batch && !POISSON ? a.table->g[slot] : a.in);
  const gcp in_scale = (gcp)(batch ? a.table->scale[slot] : a.in_scale);
  const gcp op = (gcp)(batch ? a.table->op[slot] : a.op);
  const gcp out_scale = (gcp)(batch ? a.table->scale[slot] : a.out_scale);
  const gcp background = (gcp)(batch ? a.table->bkg[d] : a.background);
  const gcp counts = (gcp)(batch ? a.table->cnt[d] : a.counts);
  // (a plain launch over several datasets -- the addend launch of walk_conv_adjoint_batch -- writes per-dataset images)
  const gp out = (gp)(POISSON && batch ? a.table->g[d]
                      : XCHG && a.comp_blocks ? a.out_comp[comp]
                      : !XCHG && !POISSON && batch ? a.table->addend[d] : a.out);
  const gp npred_out = (gp)a.npred_out;

  // taps -> SGPRs
  float tu[WK], tv[WK];
  {
    if (((int)op[0] != 1 || (int)op[1] > WK) && lane == 0) *a.guard = 1;  // not a rank-1 operator, or one whose own header asks for a wider frame (a registered buffer overwritten in place): the host reports it at its next call
    // (frame position t holds the stored tap t - WH - oy0: an operator whose PSF was embedded in a larger array of
    // zeros has its non-zero taps inside the frame the host chose for it, the taps outside are the zeros)
    float mu = 0.f, mv = 0.f;
    const int iu = lane - (WH + a.oy0), iv = lane - (WH + a.ox0);
    if (iu >= 0 && iu < a.kh) mu = op[a.taps_u + iu];
    if (iv >= 0 && iv < a.kw) mv = op[a.taps_v + iv];
#pragma unroll
    for (int t = 0; t < WK; ++t) {
      tu[t] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mu), t));
      tv[t] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mv), t));
    }
  }

  // the column taps once more, two per VGPR pair, for the packed FMAs of the column pass at 4 columns per lane (two
  // columns per lane in the 17-tap frame: scalar FMAs on the SGPR taps -- those kernels live on 128 registers; the
  // 33-tap frame has the registers of two waves per SIMD anyway); the empty asm keeps the compiler from moving the
  // (uniform) values back to SGPRs
  constexpr bool PK = C == 4 || WKT == 33;
  v2f tup[PK ? (WK + 1) / 2 : 1];
  if constexpr (PK) {
#pragma unroll
    for (int j = 0; j < (WK + 1) / 2; ++j) {
      float lo = tu[2 * j], hi = 2 * j + 1 < WK ? tu[2 * j + 1] : 0.f;
      asm volatile("" : "+v"(lo), "+v"(hi));
      tup[j] = v2f{lo, hi};
    }
  }

  const int X0 = sx * 64 * C;
  const int xm = X0 - WH + C * lane;           // image column of the lane's piece of the window
  const int xe = X0 - WH + 64 * C + C * lane;  // right-hand halo piece (lanes < NX)
  const int xo = X0 + C * lane;                // the lane's output columns
  const bool vm = xm >= 0 && xm < a.W, ve = lane < NX && xe < a.W, vo = xo < a.W;
  // lanes without a halo piece re-load the piece of lane (lane % NX) (same cache lines) and store it behind the window:
  // every lane issues the same loads and stores in every step, no branch -- the compiler can then count the loads in
  // flight exactly (s_waitcnt vmcnt(n)) instead of draining them at every merge point
  const int xd = X0 - WH + 64 * C + C * (lane % NX);
  const unsigned om = vm ? xm : 0, oe = ve ? xe : (xd < a.W ? xd : 0), oo = vo ? xo : 0;
  const int Y0 = ty * rows, y_end = min(Y0 + rows, a.H);
  const int r_begin = Y0 - WH, r_end = min(y_end + WH, a.H);  // image rows >= H contribute nothing
  float* rb = CH ? chain_lds + wv * (2 * 64 * C) : rowbuf[wv];
  // CH: this wave's stash (waves > 0) and the one of its lower neighbour, whose first walked row is image row hand0
  constexpr int SROWS = 2 * WH;
  float* const stash_w = chain_lds + L * (2 * 64 * C) + (wv - 1) * (SROWS * 64 * C) + C * lane;
  const float* const stash_r = chain_lds + L * (2 * 64 * C) + wv * (SROWS * 64 * C) + C * lane;
  const bool stash_on = CH && wv > 0, has_next = CH && wv + 1 < L && ty + 1 < tiles_y;
  const int hand0 = Y0 + rows - WH;
  constexpr int HAND_I = WS - SROWS;  // rotation state of the first handed-over step (tiles of k WS - 2 WH rows)
  bool hand_now = false, stash_now = false;  // (wave-uniform, set per round) this round ends on the handed-over rows / stashes

  struct Row { vC a, s, xa, xs; };
  struct Epi { vC p, q; };  // POISSON: background, counts; plain: out_scale, previous out
  auto row_ok = [&](int rr) { return rr >= 0 && rr < r_end; };
  // (rows outside [0, r_end) are loaded from the nearest row inside -- cache hits -- and never used)
  auto load_row = [&](int rr, Row& w) {
    const size_t base = (size_t)min(max(rr, 0), r_end - 1) * a.W;
    const gcp pin = in + base;
    w.a = *(gcv)(pin + om);
    if (IN_SCALE) w.s = *(gcv)(in_scale + base + om);
#ifdef JD_WALK_MASKED_HALO
    if (lane < NX)  // only the NX lanes with a halo piece load (and the compiler's load count becomes a bound)
#endif
    {
      w.xa = *(gcv)(pin + oe);
      if (IN_SCALE) w.xs = *(gcv)(in_scale + base + oe);
    }
  };
  auto epi_ok = [&](int y) { return y >= Y0 && y < y_end; };
  auto load_epi = [&](int y, Epi& e) {
    const size_t base = (size_t)min(max(y, Y0), y_end - 1) * a.W;
    if (POISSON) {
      e.p = *(gcv)(background + base + oo);
      e.q = *(gcv)(counts + base + oo);
    } else {
      if (out_scale) e.p = *(gcv)(out_scale + base + oo);
      if (!XCHG && a.accumulate) e.q = *(gcv)(out + base + oo);
    }
  };

  // WS = 18 accumulator slots for the 17 live outputs: with a rotation period of 18 the prefetch registers (period P,
  // P | 18) rotate statically too -- a register that is the target of a load in flight is never moved
  v2f acc[WS][C / 2];  // (pairs of columns: the operands of the packed FMAs)
#pragma unroll
  for (int s = 0; s < WS; ++s)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[s][c / 2][c % 2] = 0.f;
  static_assert(WS % P == 0, "prefetch depth must divide the rotation period");
  Row pf[P];
  Epi ep[P];
  double loss = 0.0;

#pragma unroll
  for (int p = 0; p < P; ++p) {
    load_row(r_begin + p, pf[p]);
    load_epi(r_begin + p - WH, ep[p]);
  }

  // The row exchange is software-pipelined: in step i the products of row rr + 1 go to LDS and its window is READ BACK
  // at once into the other of two window register sets, and only then the FMAs of row rr run on the window that was
  // requested one step earlier -- the LDS round trip (write, read, ~200 cycles that two waves per SIMD do not hide)
  // overlaps with 100-200 FMAs.  Measured with the read-back removed (wrong results, timing only): forward launch of
  // 2048^2 x 8 125 -> 85 us, adjoint 74 -> 58 us -- the round trip was a third of the launch.  LDS operations of one wave
  // execute in order, so one row buffer per wave still does (the next row's write cannot pass this row's read).
  float W[2][NWIN];
  // (rows outside the image go through the exchange too -- clamped loads, never used: every step issues the same LDS
  // operations, so the compiler counts the ones in flight exactly instead of waiting for all of them at a join)
  // (handed -- CH only: the neighbour's h of this row, row j of its stash, arrives in w[0 .. C) in place of the window)
  auto produce = [&](int rr1, Row& nx, float (&w)[NWIN], const bool handed, const int j) {
    if (!handed) {
      // ---- products of the row -> LDS --------------------------------------------------------------------------
      vC prod = nx.a;
      if (IN_SCALE) prod = prod * nx.s;
#pragma unroll
      for (int c = 0; c < C; ++c) prod[c] = vm ? prod[c] : 0.f;
      *reinterpret_cast<vC*>(rb + C * lane) = prod;
      vC px = nx.xa;
      if (IN_SCALE) px = px * nx.xs;
#pragma unroll
      for (int c = 0; c < C; ++c) px[c] = ve ? px[c] : 0.f;
      *reinterpret_cast<vC*>(rb + 64 * C + C * lane) = px;  // (lanes >= NX: behind the window, never read)
    }
    load_row(rr1 + P, nx);  // the row P steps ahead takes this row's registers
    if (!handed) {
      wave_lds_fence();
#pragma unroll
      for (int k = 0; k < NWIN / C; ++k) {
        const vC t = *reinterpret_cast<const vC*>(rb + C * lane + C * k);
#pragma unroll
        for (int c = 0; c < C; ++c) w[C * k + c] = t[c];
      }
      wave_lds_fence();
    } else {
      const vC t = *reinterpret_cast<const vC*>(stash_r + j * (64 * C));
#pragma unroll
      for (int c = 0; c < C; ++c) w[c] = t[c];
      // (the rest of the window holds nothing on this path; said with an empty asm, or the compiler carries the values
      // of two steps ago through the branch and copies all of them at every join)
#pragma unroll
      for (int k = C; k < NWIN; ++k) asm volatile("" : "=v"(w[k]));
    }
  };
  produce(r_begin, pf[0], W[0], false, 0);

  for (int r0 = r_begin; r0 < y_end + WH + (XCHG ? XG - 1 : 0); r0 += WS) {  // (+: the last group's flush step)
    if constexpr (CH) hand_now = has_next && r0 + HAND_I == hand0, stash_now = stash_on && r0 == r_begin;
    static_for<WS>([&](auto ic) {  // (the 18 rotation states as compile-time constants: see walk_multi_kernel)
      constexpr int i = decltype(ic)::value;
      const int rr = r0 + i;
      Epi& ce = ep[i % P];
      const bool live = row_ok(rr);
      produce(rr + 1, pf[(i + 1) % P], W[(i + 1) & 1], CH && i + 1 >= HAND_I && i + 1 < WS && hand_now, i + 1 - HAND_I);
      if (live) {
        const float (&w)[NWIN] = W[i & 1];
        // ---- row pass: h[c] = sum_t tv[t] w[c + t] -----------------------------------------------------------
        float h[C];
        if (CH && i >= HAND_I && hand_now) {
#pragma unroll
          for (int c = 0; c < C; ++c) h[c] = w[c];
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) h[c] = tv[0] * w[c];
#pragma unroll
          for (int t = 1; t < WK; ++t)
#pragma unroll
            for (int c = 0; c < C; ++c) h[c] = fmaf(tv[t], w[c + t], h[c]);
        }
        if constexpr (CH && i < SROWS) {
          if (stash_now) {  // (wave-uniform) the tile's first 2 WH rows: the tile above ends on them
            vC hv;
#pragma unroll
            for (int c = 0; c < C; ++c) hv[c] = h[c];
            *reinterpret_cast<vC*>(stash_w + i * (64 * C)) = hv;
          }
        }
        v2f hp[C / 2];
#pragma unroll
        for (int c = 0; c < C; ++c) hp[c / 2][c % 2] = h[c];
        // ---- column pass, scatter form: out[rr + 8 - t] += tu[t] h; 4 columns per lane: on packed FMAs (the same fused
        // operation per element; with one or two waves per SIMD a packed FMA costs well under two scalar ones)
        static_for<WK>([&](auto tc) {
          constexpr int t = decltype(tc)::value, s = (i + WH - t + WS) % WS;
          if constexpr (PK) {
#pragma unroll
            for (int j = 0; j < C / 2; ++j)
              acc[s][j] = t == 0 ? pk_mul_tap<0>(tup[0], hp[j]) : pk_fma_tap<t % 2>(tup[t / 2], hp[j], acc[s][j]);
          } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
              acc[s][c / 2][c % 2] = t == 0 ? tu[0] * h[c] : fmaf(tu[t], h[c], acc[s][c / 2][c % 2]);
          }
        });
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[(i + WH) % WS][c / 2][c % 2] = 0.f;
      }

      // ---- output row y = rr - 8 is complete ------------------------------------------------------------------
      const int y = rr - WH;
      if (epi_ok(y)) {
        vC conv;
#pragma unroll
        for (int c = 0; c < C; ++c) conv[c] = acc[(i + WS - WH) % WS][c / 2][c % 2];
        const size_t off = (size_t)y * a.W;
        if (POISSON) {
          vC gvec, nvec;
          float rowsum = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float n = fmaxf(conv[c], 0.f) + ce.p[c];  // clip, then the un-convolved background (npred.py:191)
            float term, g;
            poisson_point(n, ce.q[c], a.eps, a.inv_n, term, g);
            rowsum += term;
            nvec[c] = n;
            gvec[c] = conv[c] >= 0.f ? g : 0.f;  // clamp backward
          }
          if (vo) {
            loss += (double)rowsum;
            if (a.write_grad) *(gv)(out + off + oo) = gvec;
            if (npred_out) *(gv)(npred_out + off + oo) = nvec;
          }
        } else {
          vC pv;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            pv[c] = a.coef * conv[c];
            if (out_scale) pv[c] = pv[c] * ce.p[c];
          }
          if (!XCHG) {
            if (a.accumulate) pv = ce.q + pv;
            if (vo) *(gv)(out + off + oo) = pv;
          } else if constexpr (XCHG) {
            const int k = (y - Y0) / XG, gy = (i + WS - 2 * WH) % XG;  // (tiles start on a group boundary: gy is static)
            *reinterpret_cast<vC*>(xbuf + (size_t)((((k & 1) * XG + gy) * XWT + wv) * 64 + lane) * C) = pv;
          }
        }
      }
      if constexpr (XCHG) {
        // Every vector-memory operation of the exchange sits at a STATIC place of the unrolled loop and is issued by every
        // wave, needed or not (rows clamped into the tile): the compiler counts the loads in flight exactly and never has
        // to drain the prefetched rows to get at the gradient row.
        const int gy = (i + WS - 2 * WH) % XG;
        const int mine = wv < XG ? wv : XG - 1;  // the row of a group this wave adds up (waves >= XG: unused duplicates)
        if (gy == 0) {
          const int yy = min(max(y + mine, Y0), y_end - 1);
          oprev = *(gcv)(out + (size_t)yy * a.W + oo);
        }
        if (gy == XG - 1 && y - gy >= Y0 && y - gy < y_end) {  // (block-uniform) the group is complete
          __syncthreads();
          const int k = (y - Y0) / XG, yy = y - gy + mine;
          vC res = oprev;
          for (int dd = 0; dd < nb; ++dd) {
            const vC pd = *reinterpret_cast<const vC*>(xbuf + (size_t)((((k & 1) * XG + mine) * XWT + dd) * 64 + lane) * C);
            res = dd == 0 && !a.accumulate ? pd : res + pd;
          }
          if (vo && wv < XG && yy < y_end) *(gv)(out + (size_t)yy * a.W + oo) = res;
        }
      }
      load_epi(y + P, ce);
    });
    if constexpr (CH) {
      if (r0 == r_begin) __syncthreads();  // every stash of the block is complete; the first hand-over comes later
    }
  }
  if (POISSON) {
    loss = wave_sum(loss);
    // (a launch over both frames has two tilings: every dataset's row of partial sums is `part_stride` long, and the
    // entries beyond its own tile count are zeroed by its own waves -- exact in any summation order)
    const int stride = a.part_stride ? a.part_stride : n_tiles;
    if (lane == 0) {
      double* row = a.partials + (size_t)d * stride;
      row[tile] = loss;
      for (int t = tile + n_tiles; t < stride; t += n_tiles) row[t] = 0.0;
    }
  }
}

template <int WKT, int C, int P, bool POISSON, bool IN_SCALE, int XG, int XWT = XW>
__global__ __launch_bounds__(XG ? 64 * XWT : 64) void walk_kernel(WalkArgs a) {
  walk_body<WKT, C, P, POISSON, IN_SCALE, XG, XWT>(a, (int)blockIdx.x, a.strips, a.tiles_y, a.rows, POISSON ? 0 : a.order0);
}

}  // namespace

// ---- host helpers of walkconv.hip that the other units call ----------------------------------------------------------
constexpr int CHAIN_DEFAULT = 1, CHAIN_MIXED = 4;  // chain length of a plain launch / of the launch over both frames (walk_chain)
bool walk_enabled(int H, int W, int n);
int plan_frame(int kh, int kw, int oy, int ox);
int dataset_frame(const SepBatchTable& t, int i, int d, int kh, int kw, int oy, int ox);
int device_cus();
void walk_shape(int H, int W, int n, bool adjoint, int frame, int* C, int* rows);
int walk_chain(int dflt, int frame, int rows, bool adjoint = false);
size_t chain_lds_bytes(int L, int frame, int C);
int walk_blocks(int strips, int tiles_y, int L);
// tiles (= waves of a plain launch, blocks of an exchange launch) of one image at C columns per lane and `rows` rows per tile
inline long walk_tile_count(int H, int W, int C, int rows) { return (long)((W + 64 * C - 1) / (64 * C)) * ((H + rows - 1) / rows); }
// The plain walk <false, false> over n_grid datasets for the adjoint unit, which emits no plain instantiation.  walk_args: a
// WalkArgs (it crosses the units as a pointer).  _launch: the launch alone, inside the caller's guard check, profile scope
// and launch check; _checked: with its own (launch_walk).
void walk_plain_adjoint_launch(const void* walk_args, int frame, int C, int n_grid, hipStream_t stream);
int walk_plain_adjoint_checked(const void* walk_args, int frame, int C, int n_grid, hipStream_t stream);

namespace {

// tap addressing of one direction (frame independent: the kernels place the taps in their frame themselves); A: WalkArgs, MultiArgs
template <class A>
void walk_setup(A& a, int kh, int kw, int oy, int ox, int adjoint) {
  const SepGeom g = sep_geom(kh, kw, oy, ox, adjoint != 0);
  const int taps_off = 4 + (adjoint ? (int)((sep_conv_operator_floats() - 4) / 2) : 0);
  a.kh = kh, a.kw = kw;
  a.oy0 = g.oy0, a.ox0 = g.ox0 + g.shiftx;
  a.taps_u = taps_off, a.taps_v = taps_off + g.khp + g.shiftx;
}

inline void walk_tiles(WalkArgs& a, int C, int rows) {
  a.rows = rows;
  a.strips = (a.W + 64 * C - 1) / (64 * C);
  a.tiles_y = (a.H + rows - 1) / rows;
}

// Shape of a plain launch over `n` datasets in `frame`: walk_shape's (C, rows) -> a's tiling and chain length; returns C.
// max_waves > 0: taller tiles until the launch has no more waves than that; rows_opt > 0: the caller's tile height
// option, already tested by the caller's own rule, instead.
inline int walk_plain_shape(WalkArgs& a, int n, bool adjoint, int frame, long max_waves = 0, int rows_opt = 0) {
  int C, rows;
  walk_shape(a.H, a.W, n, adjoint, frame, &C, &rows);
  if (max_waves > 0)
    while (rows < 4096 && walk_tile_count(a.H, a.W, C, rows) * n > max_waves) rows += frame_ws(frame);
  if (rows_opt > 0) rows = rows_opt;
  walk_tiles(a, C, rows);
  a.chain = walk_chain(CHAIN_DEFAULT, frame, rows, adjoint);
  return C;
}

}  // namespace

}  // namespace jd

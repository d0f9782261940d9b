// ------------------------------------------------------------------------------------------
// Screened arg-max (max mode, upper triangular precision factors): the same result as gmm_fwd_kernel<MODE_MAX>, bit for bit,
// for a fraction of the fp32 matrix work.
//
//   1. SCREEN (gmm_screen_kernel): every (patch, component) log-likelihood is first evaluated APPROXIMATELY with
//      one fp16 MFMA product, ytilde = fp16(xbar / s_x)^T fp16(P'_k / s_k) (power-of-two scales, fp32 accumulate;
//      v_mfma_f32_32x32x16_f16 runs at
//      16x the rate of the fp32-input MFMA), together with a rigorous bound on its distance to the fp32 value:
//        |ytilde_j - y_j| <= eps |xbar| |P'_k[:, j]|,   eps = 2^-10 + 2^-22 + accumulation  (two fp16 roundings)
//        |ltilde - l|     <= B = sqrt(2 qtilde) e + e^2 / 2 (+ fp32 rounding slack),  e = eps |xbar| |P'_k|_F
//      (Cauchy-Schwarz twice; qtilde = sum_j ytilde_j^2 / 2).  Sweep 1 over the components finds
//      L = max_k (ltilde - B), a lower bound of the true maximum; sweep 2 keeps the components with
//      ltilde + B >= L.  Every other component is provably below the maximum.  Typically 2-5 of 128 survive.
//   2. The surviving (patch, component) pairs are counting-sorted by component (the bucket kernels of the
//      backward pass).
//   3. EXACT (gmm_exact_kernel): groups of 32 pairs that share P'_k are evaluated with the SAME fp32 MFMA chain,
//      mean order and epilogue as gmm_fwd_kernel (bit-identical l), and merged per patch with a 64-bit atomic max
//      on (l, lowest k wins ties) -- order independent, so the result is deterministic.
//   4. gmm_best_kernel decodes (max, arg-max) per patch and sums the values in a fixed order.
// Anything unusual -- a non-finite screening value, more survivors than the per-wave list holds -- raises a
// device flag; the dense fp32 kernel then runs (it is always enqueued and returns at once when the flag is clear)
// and overwrites the per-patch results.  No host synchronisation anywhere.
// ------------------------------------------------------------------------------------------
#include "gmm_internal.h"

namespace jd {

struct __attribute__((packed, aligned(4))) F4U {  // 16 bytes at a 4-byte aligned address: one global_load_dwordx4
  float x, y, z, w;
};

// Patch staging for the screen (one wave per tile of 32 patches, any number of waves per SIMD): mean-subtracted patches
// as fp16 B fragments in global memory, their norms, scales and validity, and the initial (max, arg-max) keys.  Inside
// the screen kernel -- one wave per SIMD, 512 registers -- this gather was a latency-bound prologue that nothing could
// overlap: 30 us of a 230 us launch at 2048^2.  As a kernel of its own it runs at the memory system's pace; the
// screen then starts with 16 coalesced 16-byte loads per lane.
__global__ __launch_bounds__(256) void gmm_stage_kernel(GmmStageArgs a) {
  use_device_shift(a);
  if (a.pcount && blockIdx.x == 0 && threadIdx.x == 0) *a.dense_count = 0;
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= a.n_tiles) return;
  const int h = lane >> 5, c = lane & 31;  // lane (h, c): image rows 2 s + h (pixel step s) of patch c
  const int n = a.n_begin + 32 * tile + c;
  const bool valid = n < a.n_end;
  const int py = valid ? n / a.nPx : 0, px = valid ? n - (n / a.nPx) * a.nPx : 0;
  const int x0 = px * a.stride - a.shift_x;  // in (-W, W)
  const int xb = x0 < 0 ? x0 + a.W : x0;     // first column of the patch in the image, in [0, W)
  const bool straight = xb + 7 < a.W;        // the 8 columns do not wrap around
  float x[32];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float* row = a.flux + (size_t)wrap(py * a.stride + 2 * s + h - a.shift_y, a.H) * a.W;
    if (straight) {  // two 16-byte loads at a 4-byte aligned address
      const F4U v0 = *reinterpret_cast<const F4U*>(row + xb), v1 = *reinterpret_cast<const F4U*>(row + xb + 4);
      x[8 * s + 0] = v0.x, x[8 * s + 1] = v0.y, x[8 * s + 2] = v0.z, x[8 * s + 3] = v0.w;
      x[8 * s + 4] = v1.x, x[8 * s + 5] = v1.y, x[8 * s + 6] = v1.z, x[8 * s + 7] = v1.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[8 * s + e] = row[wrap(x0 + e, a.W)];
    }
  }
  bool sel = true;
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    x[i] = valid ? x[i] : 0.f;
    sum += x[i];
    sel = sel && (x[i] > -1e5f);  // patches/core.py:215
  }
  const float mean = (sum + __shfl_xor(sum, 32, 64)) * (1.f / 64.f);
  float n2 = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) x[i] -= mean, n2 = fmaf(x[i], x[i], n2);
  n2 += __shfl_xor(n2, 32, 64);
  const int sel_other = __shfl_xor((int)sel, 32, 64);  // unconditional: see gmm_fwd_kernel
  sel = sel && sel_other != 0;
  const bool ok = valid && sel;
  // fp16 operand: xbar / s_x with the power of two s_x that puts max |xbar| into [2^13, 2^14) -- the scaling is
  // exact, nothing overflows (fp16 max 65504), and whatever underflows is below 2^-27 of the largest pixel
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(x[i]));
  amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
  int ex = 14;
  if (amax > 0.f && amax < 3.0e38f) (void)frexpf(amax, &ex);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    f16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (_Float16)ldexpf(x[8 * s + e], 14 - ex);
    a.xfrag[((size_t)tile * 4 + s) * 64 + lane] = __builtin_bit_cast(uint4, v);
  }
  if (h == 0) {
    a.xn[tile * 32 + c] = __builtin_sqrtf(n2) * 1.0001f;
    a.xs2[tile * 32 + c] = ldexpf(1.f, 2 * (ex - 14));
    a.ok[tile * 32 + c] = ok ? 1 : 0;
    if (valid) a.best[n] = ok ? best_key(-INFINITY, 0) : 0ull;
    if (valid && a.pcount) a.pcount[n] = 0, a.dense_mark[n] = 0;
  }
}

struct ScreenFrags {
  f16x8 a[A16_BLOCKS];
};

__device__ __forceinline__ void load_frags16(ScreenFrags& f, const uint4* af, int k) {
  const uint4* ak = af + (size_t)k * (A16_BLOCKS * 64);
#pragma unroll
  for (int b = 0; b < A16_BLOCKS; ++b) {
    const uint4 v = ak[b * 64];
    f.a[b] = __builtin_bit_cast(f16x8, v);
  }
}

// ytilde for one tile: coordinate block 0 (j < 32) needs pixel steps 0, 1; block 1 all four
__device__ __forceinline__ void mfma_screen(f32x16 (&acc)[2], const ScreenFrags& f, const f16x8 (&x)[4]) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[0], x[0], zero, 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[2], x[0], zero, 0, 0, 0);
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[1], x[1], acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[3], x[1], acc[1], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[4], x[2], acc[1], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[5], x[3], acc[1], 0, 0, 0);
}

// The lane's share of q = sum_j ytilde_j^2 (the 32 coordinates of its lane half)
__device__ __forceinline__ float screen_q_half(const f32x16 (&acc)[2]) {
  // two scalar fmaf chains (even / odd registers), no v_pk_fma_f32: beside MFMAs a packed fp32 instruction costs the wave more than the two scalar ones it replaces
  // (MI355X_MICROARCH.md, "price of one filler beside MFMAs"), and hipcc packs only part of them
  float q0 = 0.f, q1 = 0.f;
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      q0 = __builtin_fmaf(acc[b][r], acc[b][r], q0);
      q1 = __builtin_fmaf(acc[b][r + 1], acc[b][r + 1], q1);
    }
  return q0 + q1;
}

// TWO tiles (A, B) and one component: after the MFMAs lane (h, c) holds half of q for patch c of both tiles.  One
// v_permlane32_swap hands lanes 0-31 both halves of tile A and lanes 32-63 both halves of tile B, so the per-patch
// arithmetic below runs once for the two tiles (per-lane state: half 0 = tile A's patch, half 1 = tile B's):
//   ltilde = ck - q / 2,   |l - ltilde| <= sqrt(q) e + e^2 / 2,  e = eps |xbar| |P'_k|_F + |m'_k|
// (the screen ignores the component mean m'_k: y - m' = ytilde + d with |d| <= eps |xbar| |P'_k|_F + |m'_k|, so a
// mixture with non-zero means only gets wider bounds; the exact stage subtracts the means)
// inflated for the fp32 rounding of q, l, the hardware square root (1 ulp) and of this expression itself:
//   B = sqrt(q) * e1 + 2e-5 q + c2,   e1 = 1.001 e,   c2 = 0.5 e1^2 + 1e-6 |ck| + 1e-30.
// ONE sweep over the components: a component is recorded while its upper bound reaches the running lower bound L of
// the maximum; records made before L rose are dropped later (bucket_key) against the final L.  Visiting the
// components most-popular-first makes L rise early, so few stale records are written.
// The issue slots beside the MFMAs are the budget (about six 4-cycle VALU instructions hide per 32-cycle MFMA).
// LSE (logsumexp screen): a component is recorded while its upper bound reaches L - LSE_MARGIN -- whatever is left out is
// below exp(-25) = 1.4e-11 of the largest term of the sum, 128 components of it below 2e-9 of the sum.
constexpr float LSE_MARGIN = 25.f;
constexpr int LSE_KEEP = 28;  // candidates a patch may keep (a multiple of 4; <= LSE_ROWS, and 128 x (LSE_KEEP + 1) <= SCREEN_CAP)

// the candidate records of one pair: `mask` = ballot of the candidate lanes.  The records of both pairs are written at the
// END of a component's step (one basic block for the MFMAs and the squares of a component).
__device__ __forceinline__ void screen_emit(unsigned long long mask, float ub, int n, int k, int lane, int& cnt, int32_t* rec_n,
                                            int32_t* rec_k, float* rec_ub, int cap) {
  if (mask) {
    const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    const bool cand = ((mask >> lane) & 1ull) != 0ull;  // (a lane flag kept alive across the component's step costs it two instructions)
    if (cand && pos < cap) {  // (the wave's record buffer: uniform base pointers, one 32-bit offset)
      rec_n[pos] = n;
      rec_k[pos] = k;
      rec_ub[pos] = ub;
    }
    cnt += __popcll(mask);
  }
}

template <bool LSE = false>
__device__ __forceinline__ void screen_finish_pair(const f32x16 (&accA)[2], const f32x16 (&accB)[2], float ck, float ack,
                                                   float mnorm, float efro, float xn, float s2, bool ok, float& L,
                                                   float& qacc, int& pc, int keep, unsigned long long& mask_out,
                                                   float& ub_out, unsigned long long okmask, bool live) {
  const float qa = screen_q_half(accA), qb = screen_q_half(accB);
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(qa), __float_as_uint(qb), false, false);
  // lanes 0-31: tile A, lanes 32-63: tile B; s2 = (s_x s_k)^2 undoes the power-of-two operand scales (exactly)
  const float q = (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) * s2;
  qacc += q;  // a NaN / inf anywhere ends up here and raises the fallback flag
  const float e1 = fmaf(efro, xn, mnorm);  // efro carries eps and the factor 1.001; mnorm = 1.001 |m'_k| (see above)
  const float c2 = fmaf(0.5f * e1, e1, ack);
  const float l = fmaf(-0.5f, q, ck);
  const float B = fmaf(__builtin_amdgcn_sqrtf(q), e1, fmaf(2e-5f, q, c2));
  const float ub = l + B;
  // L = max(L, l - B) as ONE v_max_f32 (fmaxf adds a canonicalising v_max in front; a NaN operand loses either way
  // and is caught through qacc)
  unsigned long long mask;
  if (LSE) {  // a patch keeps at most `keep` candidates; one more marks it for the dense kernel (its records are dropped)
    bool cand = ok && live && ub >= L - LSE_MARGIN;
    pc += cand ? 1 : 0;
    cand = cand && pc <= keep;
    mask = __ballot(cand);
  } else {
    // the ballot of the compare alone IS its lane mask; `ok` joins as a scalar AND with its own (loop-invariant) ballot --
    // the ballot of `ok && compare` goes through a v_cndmask / v_cmp_ne pair
    mask = __builtin_amdgcn_ballot_w64(ub >= L) & okmask;
  }
  asm("v_max_f32 %0, %1, %2" : "=v"(L) : "v"(L), "v"(l - B));
  mask_out = mask, ub_out = ub;  // (emitted by the caller, see screen_emit)
}

// NP = tile pairs (of 2 x 32 patches) a wave works on.  Two decompositions:
//   KSPLIT = false  every wave owns its NP pairs and walks over ALL components (fragments amortised over 128 patches,
//                   no synchronisation at all): large inputs;
//   KSPLIT = true   the four waves of a block share NP pairs and each takes every fourth component of the visiting
//                   order: a wave's sweep is four times shorter, so a small input (a rank's share of a sharded prior)
//                   still occupies every CU for a short time instead of a few CUs for the full sweep.  Every wave
//                   keeps its own running bound L_w (a valid lower bound of the maximum), the final bound is their
//                   maximum.
constexpr int SCREEN_RB = 512;      // records a wave buffers in LDS before it writes them out (>= 2 x 64)
// KC_LDS: (k, c_k, eps |P'_k|_F, s_k^2, |m'_k|) of the component at every position of the visiting order are staged in
// LDS once per block (K <= SCREEN_KC_MAX).  The kernel stores records, so hipcc may not use scalar loads for these
// uniform values; as vector loads from global memory their latency was exposed once per component (a load of
// korder[kk + 1] followed at once by the wait for it).  From LDS they are fetched TWO positions ahead, so that the
// component index is in a register a whole component before the fragment prefetch needs it for its address.
template <int NP, bool KSPLIT, bool KC_LDS, bool LSE = false, bool CLOCK = false>
__global__ __launch_bounds__(256, NP == 1 ? 2 : 1) void gmm_screen_kernel(GmmScreenArgs a) {
  constexpr int NT = 2 * NP;
  unsigned long long clock_t0 = 0, clock_r0 = 0;
  if (CLOCK) clock_t0 = __builtin_amdgcn_s_memtime(), clock_r0 = __builtin_amdgcn_s_memrealtime();
  __shared__ float st_L[KSPLIT ? 4 * NT * 32 : 1];
  // Candidate records are collected in a wave-private LDS buffer and written to the wave's segment in global memory
  // in bulk: a global store inside the sweep is counted by vmcnt like a load, and the compiler -- which cannot know
  // whether the conditional stores were issued -- makes every later wait for the fragment prefetch drain them as well
  // (the waves were parked on s_waitcnt for a fifth of their cycles).
  __shared__ int32_t rb_n[4][SCREEN_RB], rb_k[4][SCREEN_RB];
  __shared__ float rb_ub[4][SCREEN_RB];
  __shared__ int kc_k[KC_LDS ? SCREEN_KC_MAX : 1];
  __shared__ float4 kc_f[KC_LDS ? SCREEN_KC_MAX : 1];
  __shared__ float kc_a[KC_LDS ? SCREEN_KC_MAX : 1];  // 1e-6 |c_k| + 1e-30: the rounding slack of the bound
  if (KC_LDS) {
    for (int i = threadIdx.x; i < a.K; i += 256) {
      const int k = a.korder[i];
      kc_k[i] = k;
      kc_f[i] = make_float4(a.const_k[k], a.efro_k[k], a.sk2_k[k], a.mnorm_k[k]);
      kc_a[i] = fmaf(1e-6f, fabsf(a.const_k[k]), 1e-30f);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wave_global = blockIdx.x * 4 + wave;
  const int tile0 = (KSPLIT ? (int)blockIdx.x : wave_global) * NT;  // first of this wave's (block's) NT tiles
  const int base = a.n_begin + tile0 * 32;
  const int h = lane >> 5, c = lane & 31;  // lane (h, c): image rows 2 s + h (pixel step s) of patch c
  float xn[NT], xs2[NT];
  bool ok[NT];
  int nidx[NT];
  f16x8 xf[NT][4];  // the B fragments of the wave's tiles stay in registers for the whole sweep
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int s = 0; s < 4; ++s) xf[t][s] = __builtin_bit_cast(f16x8, a.xfrag[((size_t)(tile0 + t) * 4 + s) * 64 + lane]);
    xn[t] = a.xn[(tile0 + t) * 32 + c], xs2[t] = a.xs2[(tile0 + t) * 32 + c], ok[t] = a.ok[(tile0 + t) * 32 + c] != 0;
    nidx[t] = base + 32 * t + c;
  }
  if (KC_LDS) __syncthreads();  // the constants table
  const uint4* af = a.afrag16 + lane;
  const int seg = __builtin_amdgcn_readfirstlane(wave_global * SCREEN_CAP);
  int32_t* seg_n = a.rec_n + seg;
  int32_t* seg_k = a.rec_k + seg;
  float* seg_ub = a.rec_ub + seg;
  int cnt = 0;    // records already written to the wave's global segment (may exceed SCREEN_CAP: overflow -> fallback)
  int cnt_l = 0;  // records in the LDS buffer
  int32_t* const lb_n = rb_n[wave];
  int32_t* const lb_k = rb_k[wave];
  float* const lb_ub = rb_ub[wave];
  // room for one more emission of up to 64 records?  otherwise write the buffer out (wave-uniform, rare)
  auto flush = [&](bool force) {
    if (!force && cnt_l <= SCREEN_RB - 128) return;  // (room for the two emissions of the next component)
    for (int i = lane; i < cnt_l; i += 64)
      if (cnt + i < SCREEN_CAP) seg_n[cnt + i] = lb_n[i], seg_k[cnt + i] = lb_k[i], seg_ub[cnt + i] = lb_ub[i];
    cnt += cnt_l;
    cnt_l = 0;
  };
  // per-lane state of the two tile pairs: lane half 0 carries the patch of tile 2 p, half 1 that of tile 2 p + 1
  float pxn[NP], pL[NP], pq[NP], ps2[NP];
  bool pok[NP];
  int pn[NP];
  int pc[NP];  // (logsumexp screen) candidates of the lane's patch so far
  unsigned long long okm[NP];  // ballot of pok
  // candidates a patch may keep: 30 x 128 patches fit a wave's record list, and the four waves of a KSPLIT block, which
  // share the patches, stay below the 32 rows of the patch table together
  const int keep = KSPLIT ? LSE_KEEP / 4 : LSE_KEEP;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    ps2[p] = h ? xs2[2 * p + 1] : xs2[2 * p];
    pxn[p] = h ? xn[2 * p + 1] : xn[2 * p];
    pok[p] = h ? ok[2 * p + 1] : ok[2 * p];
    pn[p] = h ? nidx[2 * p + 1] : nidx[2 * p];
    pL[p] = -INFINITY;
    pq[p] = 0.f;
    pc[p] = 0;
    okm[p] = __ballot(pok[p]);
  }

  ScreenFrags f0, f1;
  f32x16 acc[2][2][2];  // [buffer][tile of the pair][coordinate block]: one pair on the matrix pipe, one in the epilogue
  auto issue_pair = [&](f32x16 (&buf)[2][2], const ScreenFrags& f, int p) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      mfma_screen(buf[u], f, xf[2 * p + u]);
    }
  };
  constexpr int KSTEP = KSPLIT ? 4 : 1;
  const int kk0 = KSPLIT ? wave : 0;  // position in the visiting order: wave w takes w, w + 4, ...
  // (component, constants) at a position of the visiting order
  struct KConst {
    int k;
    float ck, ef, sk2, mn, ack;
  };
  auto fetch_consts = [&](int pos) {
    KConst r;
    if (KC_LDS) {
      r.k = kc_k[pos];
      const float4 c4 = kc_f[pos];
      r.ck = c4.x, r.ef = c4.y, r.sk2 = c4.z, r.mn = c4.w, r.ack = kc_a[pos];
    } else {
      r.k = a.korder[pos];
      r.ck = a.const_k[r.k], r.ef = a.efro_k[r.k], r.sk2 = a.sk2_k[r.k], r.mn = a.mnorm_k[r.k];
      r.ack = fmaf(1e-6f, fabsf(r.ck), 1e-30f);
    }
    return r;
  };
  auto clamp_pos = [&](int pos) { return pos < a.K ? pos : (kk0 < a.K ? kk0 : 0); };
  auto fetch_k = [&](int pos) { return KC_LDS ? kc_k[pos] : a.korder[pos]; };
  KConst cur = fetch_consts(clamp_pos(kk0));
  KConst nxt = fetch_consts(clamp_pos(kk0 + KSTEP));  // always one component ahead of `cur` ...
  load_frags16(f0, af, __builtin_amdgcn_readfirstlane(cur.k));
  load_frags16(f1, af, __builtin_amdgcn_readfirstlane(nxt.k));
  // prologue: pair 0 of the first component.  Unconditional (a wave without components computes on the clamped position and
  // drops the result): with the fragments of f0 consumed on EVERY path into the loop the compiler knows them loaded there,
  // and the first half of a component does not wait -- behind a conditional prologue it drained ALL outstanding loads at the
  // top of every other component, the prefetch of the component after next included
  issue_pair(acc[0], f0, 0);
  int k_ahead_next = fetch_k(clamp_pos(kk0 + 2 * KSTEP));
  // One component: `fa` holds its fragments, `fb` those of the next one (requested during the PREVIOUS component).  As
  // soon as the last MFMA that reads `fa` has been issued, the fragments of the component after next are requested into
  // it: 1.75 components (~3000 cycles) ahead of their first use -- with the request at the top of the component that
  // precedes the use the waves were parked on its vmcnt for a fifth of their cycles (SQ_WAIT_ANY).  The loop alternates
  // the two buffers, so no fragment is ever copied; PHASE = parity of the component within this wave's sweep.
  auto component = [&](ScreenFrags& fa, const ScreenFrags& fb, int kk, auto phase, bool live) {
    constexpr int PHASE = decltype(phase)::value;
    const int k = __builtin_amdgcn_readfirstlane(cur.k);
    const float ck = cur.ck, ef = cur.ef, sk2 = cur.sk2, mn = cur.mn;
    const float ack = cur.ack;
    const int k_ahead = k_ahead_next;                    // the component after next: read from LDS a component ago
    k_ahead_next = fetch_k(clamp_pos(kk + 3 * KSTEP));  // (consumed at once it would expose the LDS latency)
    cur = nxt;
    nxt = fetch_consts(clamp_pos(kk + 2 * KSTEP));  // ... and fetched two ahead of its use
    unsigned long long m0 = 0ull, m1 = 0ull;
    float u0 = 0.f, u1 = 0.f;
    if (NP == 2) {
      // pair 1 of k on the matrix pipe while pair 0 of k finishes in its shadow, then pair 0 of k + 1 | pair 1 of k
      issue_pair(acc[1], fa, 1);
      load_frags16(fa, af, __builtin_amdgcn_readfirstlane(k_ahead));  // unconditional (clamped) prefetch
      screen_finish_pair<LSE>(acc[0][0], acc[0][1], ck, ack, mn, ef, pxn[0], ps2[0] * sk2, pok[0], pL[0], pq[0], pc[0], keep,
                              m0, u0, live ? okm[0] : 0ull, live);
      issue_pair(acc[0], fb, 0);
      screen_finish_pair<LSE>(acc[1][0], acc[1][1], ck, ack, mn, ef, pxn[NP - 1], ps2[NP - 1] * sk2, pok[NP - 1], pL[NP - 1],
                              pq[NP - 1], pc[NP - 1], keep, m1, u1, live ? okm[NP - 1] : 0ull, live);
    } else {
      // the only pair of k + 1 on the matrix pipe while the pair of k finishes; the accumulator buffers alternate
      load_frags16(fa, af, __builtin_amdgcn_readfirstlane(k_ahead));  // (fa's MFMAs were issued by the previous component)
      issue_pair(acc[1 - PHASE], fb, 0);
      screen_finish_pair<LSE>(acc[PHASE][0], acc[PHASE][1], ck, ack, mn, ef, pxn[0], ps2[0] * sk2, pok[0], pL[0], pq[0], pc[0],
                              keep, m0, u0, live ? okm[0] : 0ull, live);
    }
    // the component's step is one scheduling region: one MFMA, then 8 vector instructions, 12 NP times --
    // the squares of one pair spread under the MFMAs of the other (left alone, the scheduler bunches the second pair's
    // MFMAs behind its predecessor's epilogue)
    if (NP == 2 && !LSE && !KSPLIT) {
#pragma unroll
      for (int i = 0; i < 12 * NP; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
      }
    }
    // the records of the component, written behind its MFMAs and squares (SCREEN_RB holds two emissions of 64 + the
    // buffered rest: the flush check runs once per component)
    if (m0 | m1) {
      screen_emit(m0, u0, pn[0], k, lane, cnt_l, lb_n, lb_k, lb_ub, SCREEN_RB);
      if (NP == 2) screen_emit(m1, u1, pn[NP - 1], k, lane, cnt_l, lb_n, lb_k, lb_ub, SCREEN_RB);
      flush(false);
    }
  };
  // Components go in PAIRS, the loop has one exit: where a wave's share of the components is odd, the second component of
  // its last pair is the (clamped) first position once more with its records suppressed (`live`; its bound changes
  // nothing: L already holds it).  A conditional second component -- or a second exit -- leaves an edge from the end of the
  // first component to the top of the loop, on which that component's prefetch (six loads into f0) is the newest thing in
  // flight: the compiler then makes the first half of EVERY even component wait for all outstanding loads, the prefetch
  // of the component after next included (s_waitcnt vmcnt(5) ... vmcnt(0) at the loop header).
  for (int kk = kk0; kk < a.K; kk += 2 * KSTEP) {
    component(f0, f1, kk, std::integral_constant<int, 0>{}, true);
    component(f1, f0, kk + KSTEP, std::integral_constant<int, 1>{}, kk + KSTEP < a.K);
  }
  bool trouble = false;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    trouble = trouble || (pok[p] && !(pq[p] < 3.0e38f));
    if (LSE && pc[p] > keep && pn[p] < a.n_end) a.dense_mark[pn[p]] = 1;  // (several waves may store the same 1)
    if (KSPLIT)
      st_L[wave * (NT * 32) + (2 * p + h) * 32 + c] = pL[p];
    else if (pn[p] < a.n_end)
      a.lfinal[pn[p]] = pL[p];
  }
  if (KSPLIT) {  // the final lower bound of a patch is the best of the four waves' bounds
    __syncthreads();
    for (int i = threadIdx.x; i < NT * 32; i += 256)
      if (base + i < a.n_end)
        a.lfinal[base + i] = fmaxf(fmaxf(st_L[i], st_L[NT * 32 + i]), fmaxf(st_L[2 * NT * 32 + i], st_L[3 * NT * 32 + i]));
  }
  // (the counting pass of the record sort was tried here, on the wave's own records against the bound it has just
  // computed: the count kernel went away, -7 us, but at one wave per SIMD the re-read of the records is pure latency
  // and the screen grew by 22 us)
  flush(true);
  if (lane == 0) a.seg_cnt[wave_global] = cnt < SCREEN_CAP ? cnt : SCREEN_CAP;
  if (__ballot(trouble) != 0ull || cnt > SCREEN_CAP) {
    if (lane == 0) __hip_atomic_store(a.flag, a.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (CLOCK) {
    __syncthreads();  // every wave of the block is done
    if (threadIdx.x == 0 && (int)blockIdx.x < a.clock_cap) {
      a.clock_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - clock_t0;
      a.clock_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - clock_r0;
    }
  }
}

#ifdef JD_EXACT_STAMPS
#define EXACT_STAMP(i)                                                              \
  do {                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                              \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                     \
    __builtin_amdgcn_sched_barrier(0);                                              \
    if (lane == 0) a.stamps[(size_t)grp * 8 + (i)] = t_;                            \
  } while (0)
#else
#define EXACT_STAMP(i) do {} while (0)
#endif

constexpr int EXACT_PITCH = 68;  // floats per staged patch (64 + pad: 16-byte aligned rows, 2-way bank spread)
constexpr int EXACT_DRAW = 1;  // groups a wave draws from the work counter at a time
constexpr int EXACT_OFF_LDS = 1025;        // bucket offsets kept in LDS up to K = 1024

// l(n, k) exactly as gmm_fwd_kernel computes it (same mean order, same MFMA chains, same epilogue), for groups of 32
// surviving records that share the component; merged per patch with an order-independent atomic max.  The patches
// of a group are fetched with 16-byte row segments into a wave-private LDS image (the per-pixel gather of the
// backward kernel costs 4x the memory instructions) and read back in B-operand order.
template <bool TRI>
__global__ __launch_bounds__(256) void gmm_exact_kernel(GmmExactArgs a) {
  use_device_shift(a);
  if (*a.flag == a.gen) return;  // the dense kernel takes over
  __shared__ __attribute__((aligned(16))) float stage[4][32 * EXACT_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, n16 = lane & 15;
  const int wave_global = blockIdx.x * 4 + wave;
  const int n_waves = gridDim.x * 4;
  const int n_groups = a.offsets[a.K] >> 5;
  float* st = stage[wave];
  // Work distribution.  Phase stamps of the groups (diagnostic build -DJD_EXACT_STAMPS, profiles/r03/exact_stamps.txt): a
  // group takes 36 k cycles where its two products need 5 k -- dependent memory round trips at ~2 us each under load --
  // with a q90 / q50 spread of 1.7 in every phase, so with a fixed run of 4 groups per wave the launch lasts as long as
  // its unluckiest wave (85 us against 55 us per wave on average).  A block therefore owns a contiguous run of groups
  // (one or two components: their fragments stay in this CU's L1) and its four waves DRAW them, EXACT_DRAW at a time,
  // from a counter in LDS; the bucket offsets they search sit in LDS too.  (One global counter for all waves was
  // measured at 137-207 us: 3072 returning atomics on one address serialise at ~40 ns each.)  Results do not depend on
  // who evaluates a group (atomicMax merge, gradient rows by bucket slot).
  (void)n_waves, (void)wave_global;
  __shared__ int s_off[EXACT_OFF_LDS];
  __shared__ int s_next;
  const bool off_lds = a.K + 1 <= EXACT_OFF_LDS;
  const int per_block = (n_groups + (int)gridDim.x - 1) / (int)gridDim.x;
  const int b_begin = (int)blockIdx.x * per_block, b_end = b_begin + per_block < n_groups ? b_begin + per_block : n_groups;
  if (threadIdx.x == 0) s_next = b_begin;
  if (off_lds)
    for (int i = threadIdx.x; i <= a.K; i += 256) s_off[i] = a.offsets[i];
  __syncthreads();
  auto offset_of = [&](int kk) { return off_lds ? s_off[kk] : a.offsets[kk]; };
  int k = -1;
  float ck = 0.f;
  float4 A[4][4], M[4];
  for (;;) {
    int g_begin = 0;
    if (lane == 0) g_begin = atomicAdd(&s_next, EXACT_DRAW);
    g_begin = __builtin_amdgcn_readfirstlane(g_begin);
    if (g_begin >= b_end) break;  // (every wave ends here: the counter only grows)
    const int g_end = g_begin + EXACT_DRAW < b_end ? g_begin + EXACT_DRAW : b_end;
  for (int grp = g_begin; grp < g_end; ++grp) {
    EXACT_STAMP(0);  // group start
    int kg = k;
    if (kg < 0 || offset_of(kg) > 32 * grp || offset_of(kg + 1) <= 32 * grp) {
      // the last k with offsets[k] <= 32 grp (buckets are padded to 32: no straddling)
      int lo = 0, hi = a.K;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offset_of(mid) <= 32 * grp) lo = mid; else hi = mid;
      }
      kg = lo;
    }
    if (kg != k) {
      k = kg;
      ck = a.const_k[k];
      const float4* ak = reinterpret_cast<const float4*>(a.afrag) + (size_t)k * (AFRAG_FLOATS / 4) + lane;
      const float4* mk = reinterpret_cast<const float4*>(a.mfrag) + (size_t)k * 16 + g;
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        M[jb] = mk[jb * 4];
#pragma unroll
        for (int st4 = 0; st4 < 4; ++st4)
          if (!TRI || st4 <= jb) A[jb][st4] = ak[(jb * 4 + st4) * 64];
      }
    }
    const int nvalid = a.counts[k] - (32 * grp - offset_of(k));  // >= 1
#ifdef JD_EXACT_STAMPS
    if (lane == 0) a.stamps[(size_t)grp * 8 + 7] = (unsigned long long)((nvalid << 8) | (k & 255));
    { float touch = A[0][0].x + M[0].x; asm volatile("" ::"v"(touch)); }  // the fragment loads have arrived
#endif
    EXACT_STAMP(1);  // bucket found, fragments of a new component in registers
    // ---- stage: lane (q = lane / 2, hh = lane % 2) fetches columns 4 hh .. 4 hh + 3 of the 8 rows of record q
    {
      const int q = lane >> 1, hh = lane & 1;
      const bool have = q < nvalid;
      const int n = have ? a.order_n[32 * grp + q] : 0;
      const int py = n / a.nPx, px = n - py * a.nPx;
      const int x0 = px * a.stride + 4 * hh - a.shift_x;  // in (-W, W)
      const bool straight = x0 >= 0 && x0 + 3 < a.W;
      const int xw[4] = {wrap(x0, a.W), wrap(x0 + 1, a.W), wrap(x0 + 2, a.W), wrap(x0 + 3, a.W)};
      float4 rows[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float* row = a.flux + (size_t)wrap(py * a.stride + r - a.shift_y, a.H) * a.W;
        if (straight) {
          const F4U v = *reinterpret_cast<const F4U*>(row + x0);
          rows[r] = make_float4(v.x, v.y, v.z, v.w);
        } else {
          rows[r] = make_float4(row[xw[0]], row[xw[1]], row[xw[2]], row[xw[3]]);
        }
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) *reinterpret_cast<float4*>(st + q * EXACT_PITCH + 8 * r + 4 * hh) = rows[r];
    }
    EXACT_STAMP(2);  // record indices read, patch rows fetched and stored to LDS
    int n[2];
    bool valid[2];
    float x[2][16];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int q = 16 * nb + n16;
      valid[nb] = q < nvalid;
      n[nb] = valid[nb] ? a.order_n[32 * grp + q] : 0;
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) x[nb][s4] = valid[nb] ? st[q * EXACT_PITCH + 4 * s4 + g] : 0.f;
      const float mean = patch_mean_groups(x[nb]);
#pragma unroll
      for (int s4 = 0; s4 < 16; ++s4) x[nb][s4] -= mean;
    }
#ifdef JD_EXACT_STAMPS
    { float touch = x[0][0] + x[1][15]; asm volatile("" ::"v"(touch)); }
#endif
    EXACT_STAMP(3);  // patches read back from LDS, means subtracted
    f32x4 y[4][2];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      y[jb][0] = y[jb][1] = f32x4{M[jb].x, M[jb].y, M[jb].z, M[jb].w};
#pragma unroll
      for (int st4 = 0; st4 < 4; ++st4) {
        if (TRI && st4 > jb) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
            y[jb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(A[jb][st4], e), x[nb][4 * st4 + e], y[jb][nb], 0, 0, 0);
      }
    }
#ifdef JD_EXACT_STAMPS
    { float touch = y[3][1][3] + y[0][0][0]; asm volatile("" ::"v"(touch)); }
#endif
    EXACT_STAMP(4);  // first product (40 x 2 MFMAs) done
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const float l = fmaf(-0.5f, sum_lane_groups(sum_squares(y, nb)), ck);  // = finish_tile of the forward kernel
      const int tie = a.grec ? 32 * grp + 16 * nb + n16 : k;
      if (a.lrec) {
        if (g == 0 && valid[nb]) a.lrec[32 * grp + 16 * nb + n16] = l;
      } else if (g == 0 && valid[nb] && l > -INFINITY) {
        atomicMax(a.best + n[nb], best_key(l, tie));  // NaN never wins (l > b)
      }
    }
    EXACT_STAMP(5);  // value epilogue, atomicMax issued
    if (a.grec) {
      float* rows[2] = {a.grec + (size_t)(32 * grp + n16) * D, a.grec + (size_t)(32 * grp + 16 + n16) * D};
      patch_gradient_rows<TRI>(y, a.gfrag, k, lane, valid, rows);
    }
#ifdef JD_EXACT_STAMPS
    __builtin_amdgcn_s_waitcnt(0);  // the gradient rows have left the wave
#endif
    EXACT_STAMP(6);  // second product + gradient rows stored
  }
  }
}

constexpr int BEST_CHUNK = 1024;

__global__ __launch_bounds__(256) void gmm_best_kernel(GmmBestArgs a) {
  use_device_shift(a.fb);
  __shared__ double red[4];
  const int base = a.n_begin + blockIdx.x * BEST_CHUNK;
  const bool slots = a.winner && *a.flag != a.gen;
  double local = 0.0;
  // (the block's keys by unconditional loads, all in flight at once: under the bounds test the compiler emitted load, wait,
  // store, wait per 256 patches -- eight dependent round trips in a launch of one block per CU)
  unsigned long long keys[BEST_CHUNK / 256];
#pragma unroll
  for (int i = 0; i < BEST_CHUNK / 256; ++i) {
    const int n = base + i * 256 + threadIdx.x;
    keys[i] = a.best[n < a.n_end ? n : a.n_end - 1];
  }
  if (slots && !a.argmax_out) {  // (block-uniform) the fit's path: nothing but the winner slots to store, no loads in the loop
#pragma unroll
    for (int i = 0; i < BEST_CHUNK / 256; ++i) {
      const int n = base + i * 256 + threadIdx.x;
      if (n < a.n_end) {
        const unsigned long long key = keys[i];
        const bool ok = key != 0ull;
        const float v = best_value(key);
        a.winner[n] = ok && v > -INFINITY ? best_component(key) : -1;
        if (ok) local += (double)v;
      }
    }
  } else
#pragma unroll
  for (int i = 0; i < BEST_CHUNK / 256; ++i) {
    const int n = base + i * 256 + threadIdx.x;
    if (n < a.n_end) {
      const unsigned long long key = keys[i];
      const bool ok = key != 0ull;
      const float v = best_value(key);
      int k = ok ? best_component(key) : -1;
      if (slots) {
        const int slot = ok && v > -INFINITY ? k : -1;  // no record won: component 0 like the plain keys, no gradient
        a.winner[n] = slot;
        if (a.argmax_out) k = ok ? (slot >= 0 ? a.rec_k[a.rec_order[slot]] : 0) : -1;
      } else if (a.argmax_fb) {
        a.argmax_fb[n] = k;
      }
      if (a.argmax_out) a.argmax_out[n] = k;
      if (ok) local += (double)v;
    }
  }
  local = wave_sum(local);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (a.fb.gpatch && !slots && a.winner) {  // (block-uniform: the pass fell back to the dense kernel)
    __syncthreads();                        // this block's argmax_fb entries are written
    const int grp0 = blockIdx.x * (BEST_CHUNK / 32);
    const int n_groups = (a.n_end - a.n_begin + 31) >> 5;
    const int grp1 = grp0 + BEST_CHUNK / 32 < n_groups ? grp0 + BEST_CHUNK / 32 : n_groups;
    bwd_fallback_groups<true>(a.fb, grp0 + (threadIdx.x >> 6), grp1, 4);
  }
  __shared__ int last;
  if (threadIdx.x == 0) {
    a.partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    __threadfence();  // the partial sum is visible device-wide before the ticket is drawn
    last = atomicAdd(a.ticket, 1) == (int)gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  // finalize_sum_kernel's order: thread t adds partials t, t + 256, ..., then the fixed block reduction
  __shared__ double smem[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {
    const unsigned long long bits = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(a.partials + i),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // not through this CU's L1
    acc += __builtin_bit_cast(double, bits);
  }
  const double total = block_sum<256>(acc, smem);
  if (threadIdx.x == 0) {
    double v = a.scale * total;
    if (a.accumulate) v += (double)a.value_out[0];
    a.value_out[0] = (float)v;
    *a.ticket = 0;
    if (a.host_stats) {
      a.host_stats[1] = *a.flag == a.gen ? 1 : 0;
      a.host_stats[2] = *a.slots_used;
      a.host_stats[3] = a.n_end - a.n_begin;
      __threadfence_system();
      a.host_stats[0] = a.gen;  // last: marks the other three as belonging to this pass
    }
  }
}

// ------------------------------------------------------------------------------------------
// Logsumexp mode through the screen (marginalize = True, patches/core.py:242-243): the screen keeps every component whose
// upper bound reaches L - 25 (L = the lower bound of the patch's maximum), the exact kernel evaluates l and the
// gradient row of each surviving (patch, component) record, and this kernel combines the records of a patch:
//   v = m + log sum_j exp(l_j - m),  row = sum_j exp(l_j - m) row_j / sum_j exp(l_j - m)   (m = max_j l_j)
// in ascending order of the bucket slot (= of the component: deterministic, whatever order the scatter kernel's atomics
// listed them in).  What the screen left out is below 2e-9 of the sum.  16 lanes per patch, each with one float4 of the
// 256-byte rows; a block = 16 patches.  After a fallback (*flag == gen) the gated dense kernels have done the work.
constexpr int LSE_ROWS = 32;  // records per patch the patch table holds (more: fallback to the dense kernels)

__global__ __launch_bounds__(256) void gmm_lse_combine_kernel(GmmLseCombineArgs a) {
  __shared__ int s_slot[16][LSE_ROWS];
  __shared__ float s_l[16][LSE_ROWS];
  if (*a.flag == a.gen) return;  // (block-uniform)
  const int grp = threadIdx.x >> 4, part = threadIdx.x & 15;
  const int n = a.n_begin + (int)blockIdx.x * 16 + grp;
  const bool live = n < a.n_end && a.mark[n < a.n_end ? n : a.n_begin] == 0;
  int c = live ? a.pcount[n] : 0;
  if (c > a.rows) c = a.rows;  // (cannot be: the scatter kernel raised the flag)
  // the patch's records, two per lane; rank by bucket slot -> LDS in ascending order
  int slot[2];
  float l[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = part + 16 * u;
    slot[u] = j < c ? a.ptab[(size_t)n * a.rows + j] : 0x7fffffff;
    l[u] = j < c ? a.lrec[slot[u]] : -INFINITY;
  }
  int rank[2] = {0, 0};
  for (int j = 0; j < c; ++j) {  // (c is uniform over the 16 lanes of the patch)
    const int other = __shfl(j < 16 ? slot[0] : slot[1], (threadIdx.x & 48) + (j & 15), 64);
    rank[0] += other < slot[0] ? 1 : 0;
    rank[1] += other < slot[1] ? 1 : 0;
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (part + 16 * u < c) s_slot[grp][rank[u]] = slot[u], s_l[grp][rank[u]] = l[u];
  float m = fmaxf(l[0], l[1]);
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));  // (stays inside the 16 lanes)
  __syncthreads();
  float4 G = make_float4(0.f, 0.f, 0.f, 0.f);
  float S = 0.f;
  for (int r = 0; r < c; ++r) {
    const float e = expf(s_l[grp][r] - m);
    const float4 row = reinterpret_cast<const float4*>(a.grec + (size_t)s_slot[grp][r] * D)[part];
    S += e;
    G.x = fmaf(e, row.x, G.x), G.y = fmaf(e, row.y, G.y), G.z = fmaf(e, row.z, G.z), G.w = fmaf(e, row.w, G.w);
  }
  if (live) {
    const float inv = c > 0 ? 1.f / S : 0.f;  // (no record: a filtered patch -- no value, no gradient)
    reinterpret_cast<float4*>(a.gpatch + (size_t)(n - a.n_begin) * D)[part] = make_float4(G.x * inv, G.y * inv, G.z * inv, G.w * inv);
  }
  if (part == 0 && live) a.vpatch[n] = c > 0 ? m + logf(S) : 0.f;
}

// The marked patches of the pass, compacted: a block ranks the marks of its 1024 patches and reserves its piece of the
// list with one atomicAdd (the order of the pieces is whatever the atomics make it -- every result is stored by patch
// index, so none depends on it)
__global__ __launch_bounds__(256) void gmm_lse_list_kernel(const int* mark, int n_begin, int n_end, const int* flag, int gen,
                                                           int32_t* list, int* count) {
  __shared__ int wave_cnt[4][4];
  __shared__ int base;
  if (*flag == gen) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int first = n_begin + (int)blockIdx.x * 1024;
  bool marked[4];
  int rank[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = first + i * 256 + (int)threadIdx.x;
    marked[i] = n < n_end && mark[n] != 0;
    const unsigned long long b = __ballot(marked[i]);
    rank[i] = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[i][wave] = __popcll(b);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int c = wave_cnt[i][w];
        wave_cnt[i][w] = total;
        total += c;
      }
    base = total ? atomicAdd(count, total) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (marked[i]) list[base + wave_cnt[i][wave] + rank[i]] = first + i * 256 + (int)threadIdx.x;
}

// Partial sums of the per-patch values in a fixed order (1024 patches per block, thread t adds patches t, t + 256, ...)
// and the number of patches the dense kernel had to take
__global__ __launch_bounds__(256) void gmm_lse_value_kernel(const float* vpatch, const int* mark, int n_begin, int n_end,
                                                            double* partials, int* marked) {
  __shared__ double red[4];
  __shared__ int redm[4];
  const int base = n_begin + (int)blockIdx.x * 1024;
  double local = 0.0;
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = base + i * 256 + (int)threadIdx.x;
    const bool marked = n < n_end && mark[n] != 0;
    if (n < n_end) local += (double)vpatch[n];
    cnt += __popcll(__ballot(marked));
  }
  local = wave_sum(local);  // (cnt: the wave's marked patches, the same number in every lane)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local, redm[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    marked[blockIdx.x] = (redm[0] + redm[1]) + (redm[2] + redm[3]);
  }
}

// value_out = [value_out +] scale * sum(partials); also leaves the pass statistics for the host (see
// GmmBestArgs::host_stats): "fell back" = 1 after a fallback, 2 when the dense kernel took more than 60 % of the patches
__global__ __launch_bounds__(256) void gmm_lse_finalize_kernel(const double* partials, const int* marked, int count,
                                                               const int* flag, int gen, double scale, float* value_out,
                                                               int accumulate, int* host_stats, const int* slots_used,
                                                               int patches) {
  __shared__ double smem[4];
  __shared__ int smem_i[4];
  double acc = 0.0;
  int cnt = 0;
  for (int i = threadIdx.x; i < count; i += 256) acc += partials[i], cnt += marked[i];
  const double total = block_sum<256>(acc, smem);
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);  // patches the dense kernel took
  if ((threadIdx.x & 63) == 0) smem_i[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = scale * total;
    if (accumulate) v += (double)value_out[0];
    value_out[0] = (float)v;
    if (host_stats) {
      const int n_marked = (smem_i[0] + smem_i[1]) + (smem_i[2] + smem_i[3]);
      // (screen + sort + records cost about a third of a dense pass: beyond 60 % of the patches the dense pass alone is cheaper)
      host_stats[1] = *flag == gen ? 1 : (5 * (long)n_marked > 3 * (long)patches ? 2 : 0);
      host_stats[2] = *slots_used;
      host_stats[3] = patches;
      __threadfence_system();
      host_stats[0] = gen;
    }
  }
}

#ifdef JD_EXACT_STAMPS
// Diagnostic build: the exact kernel's launch with a stamp buffer ([group][8] s_memtime values) and, under
// JD_GMM_SCREEN_DEBUG, the phase histogram of the launch (synchronises).
static int launch_exact_stamped(jd_gmm* g, GmmExactArgs& ex, size_t slots, hipStream_t s) {
  static unsigned long long* stamps_dev = nullptr;
  static size_t stamps_cap = 0;
  const size_t max_groups = slots / 32 + g->K + 8;
  if (stamps_cap < max_groups) {
    if (stamps_dev) (void)hipFree(stamps_dev);
    JD_HIP(hipMalloc(&stamps_dev, max_groups * 8 * sizeof(unsigned long long)));
    stamps_cap = max_groups;
  }
  ex.stamps = stamps_dev;
  {
    ProfScope stage(JD_KERNEL_GMM_EXACT, s);
    gmm_exact_kernel<true><<<(unsigned)(g->n_cu * 3), 256, 0, s>>>(ex);
  }
  JD_LAUNCH_CHECK();
  if (!opt_is_set(OPT_GMM_SCREEN_DEBUG)) return JD_OK;
  JD_HIP(hipStreamSynchronize(s));
  int total_slots = 0;
  JD_HIP(hipMemcpy(&total_slots, ex.offsets + g->K, sizeof(int), hipMemcpyDeviceToHost));
  const int n_groups = total_slots >> 5;
  std::vector<unsigned long long> st((size_t)n_groups * 8);
  JD_HIP(hipMemcpy(st.data(), stamps_dev, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const char* names[6] = {"bucket + fragments", "indices + patch rows -> LDS", "LDS read-back + mean", "first product (80 MFMAs)",
                          "value epilogue + atomicMax", "second product + gradient rows"};
  double sum[6] = {0};
  std::vector<double> per[6];
  unsigned long long t_min = ~0ull, t_max = 0;
  for (int gi = 0; gi < n_groups; ++gi) {
    const unsigned long long* t = &st[(size_t)gi * 8];
    for (int ph = 0; ph < 6; ++ph) {
      const double dt = (double)(t[ph + 1] - t[ph]);
      sum[ph] += dt;
      per[ph].push_back(dt);
    }
    t_min = t[0] < t_min ? t[0] : t_min, t_max = t[6] > t_max ? t[6] : t_max;
  }
  fprintf(stderr, "[jd exact stamps] %d groups of 32 records, first stamp to last stamp %.0f shader cycles\n", n_groups,
          (double)(t_max - t_min));
  double total = 0;
  for (int ph = 0; ph < 6; ++ph) total += sum[ph];
  for (int ph = 0; ph < 6; ++ph) {
    std::sort(per[ph].begin(), per[ph].end());
    const size_t m = per[ph].size();
    fprintf(stderr, "[jd exact stamps] %-34s mean %8.0f cycles (%4.1f %%)  q10 %7.0f  q50 %7.0f  q90 %7.0f  q99 %7.0f\n", names[ph],
            sum[ph] / n_groups, 100.0 * sum[ph] / total, per[ph][m / 10], per[ph][m / 2], per[ph][m * 9 / 10], per[ph][m * 99 / 100]);
  }
  fprintf(stderr, "[jd exact stamps] per group %.0f cycles; groups per wave %.2f; waves %d\n", total / n_groups,
          (double)n_groups / (double)(g->n_cu * 12), g->n_cu * 12);
  return JD_OK;
}
#endif

static int launch_exact(jd_gmm* g, GmmExactArgs& ex, size_t slots, hipStream_t s) {
#ifdef JD_EXACT_STAMPS
  return launch_exact_stamped(g, ex, slots, s);
#else
  {
    ProfScope stage(JD_KERNEL_GMM_EXACT, s);
    gmm_exact_kernel<true><<<(unsigned)(g->n_cu * 3), 256, 0, s>>>(ex);
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
#endif
}

// Max mode through the fp16 screen (see gmm_screen_kernel): fills a.argmax_out (if any) and one fp64 partial sum per
// 1024 patches, exactly the numbers gmm_fwd_kernel<MODE_MAX> produces.
// fused: the exact kernel also writes the gradient row of every surviving record and gmm_best_kernel the winning row
// of every patch (g->fused.grec, g->fused.winner); after a fallback the components are in fallback_argmax instead.
// lse: logsumexp mode (always with the gradient; see gmm_lse_combine_kernel): the screen keeps the components within
// LSE_MARGIN of the lower bound, the exact kernel stores l per record, the combine kernel turns the records of a patch
// into its value and its gradient row (g->dense.gpatch); the dense logsumexp kernels are enqueued behind the device flag.
int screened_forward(jd_gmm* g, const GmmFwdArgs& a, hipStream_t s, int* n_partials, bool fused, int32_t* fallback_argmax,
                     double value_scale, float* value_out, int accumulate_value, bool lse) {
  jd_gmm::Screen& sn = g->screen;
  const long n = a.n_end - a.n_begin;
  // every wave its own 128 patches and all components, unless that leaves CUs without a block: then the four waves of
  // a block share 128 patches and split the components (see gmm_screen_kernel)
  bool ksplit = (n + SCREEN_T * 32 * 4 - 1) / (SCREEN_T * 32 * 4) < g->n_cu;
  if (opt_is_set(OPT_GMM_KSPLIT)) ksplit = opt_value(OPT_GMM_KSPLIT, 0) != 0;  // testing: force either decomposition
  constexpr int T = SCREEN_T;
  const unsigned blocks = (unsigned)(ksplit ? (n + T * 32 - 1) / (T * 32) : ((n + T * 32 - 1) / (T * 32) + 3) / 4);
  const size_t n_seg = (size_t)blocks * 4;
  const size_t slots = n_seg * SCREEN_CAP;                  // candidate record slots
  const size_t bucket_slots = slots + 32 * (size_t)g->K;    // padded bucket slots
  JD_REQUIRE(bucket_slots < (size_t)1 << 31, "jd_gmm_prior_fwd_bwd: too many patches for the screened path");
  int rc;
  if ((rc = sn.best.reserve((size_t)a.n_end))) return rc;
  if ((rc = sn.lfinal.reserve((size_t)a.n_end))) return rc;
  if ((rc = sn.rec.reserve(3 * slots))) return rc;
  if ((rc = sn.rec_order.reserve(bucket_slots))) return rc;
  if ((rc = sn.rec_order_n.reserve(bucket_slots))) return rc;
  if ((rc = sn.seg_cnt.reserve(n_seg))) return rc;
  if ((rc = g->dense.partials.reserve((size_t)((n + 31) / 32 + 4)))) return rc;
  int32_t* rec_n = sn.rec.ptr;
  int32_t* rec_k = sn.rec.ptr + slots;
  float* rec_ub = reinterpret_cast<float*>(sn.rec.ptr + 2 * slots);
  int* flag = sn.ctl.ptr;
  sn.gen = sn.gen % (1 << 30) + 1;
  // a pass whose shifts come from device memory may be REPLAYED from a captured graph with this very generation number:
  // a fallback flag left by an earlier replay must not be taken for this pass's (a node of the graph clears it)
  if (a.shift_dev) JD_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
  // rows of the record-gradient buffer: 1.0-1.3 records per patch survive on the seeded mixtures of the benchmark, up
  // to 1.9 on noise under an image-like mixture (condition numbers 1e5: wider bounds); beyond 4 per patch (+ bucket
  // padding; 1 KB per patch) the scan kernel raises the fallback flag and the dense kernel takes the pass
  if (fused && g->fused.stats.host) {
    volatile int* hs = g->fused.stats.host;
    const int seen = hs[0];
    if (seen != g->fused.stats_seen_gen && seen > 0) {  // a pass has finished since the last look
      const long used = hs[2], patches = hs[3];
      if (patches > 0 && (hs[1] != 0 || used - 32L * g->K > (long)(0.6 * g->fused.rows_per_patch * (double)patches)) &&
          g->fused.rows_per_patch < 32)
        g->fused.rows_per_patch *= 2;
      g->fused.stats_seen_gen = seen;
    }
  }
  const size_t grec_rows = fused ? (size_t)g->fused.rows_per_patch * (size_t)n + 32 * (size_t)g->K : 0;
  if (fused) {
    if ((rc = g->fused.grec.reserve(grec_rows * D))) return rc;
    if ((rc = g->fused.winner.reserve((size_t)a.n_end))) return rc;
  }
  const unsigned combine_blocks = (unsigned)((n + 15) / 16), value_blocks = (unsigned)((n + 1023) / 1024);
  if (lse) {
    if ((rc = g->lse.lrec.reserve(bucket_slots))) return rc;
    if ((rc = g->lse.pcount.reserve((size_t)a.n_end))) return rc;
    if ((rc = g->lse.dense_mark.reserve((size_t)a.n_end))) return rc;
    if ((rc = g->lse.vpatch.reserve((size_t)a.n_end))) return rc;
    if ((rc = g->lse.ptab.reserve((size_t)a.n_end * LSE_ROWS))) return rc;
    if ((rc = g->lse.partials.reserve((size_t)value_blocks))) return rc;
    if ((rc = g->lse.marked.reserve((size_t)value_blocks))) return rc;
    if ((rc = g->lse.dense_list.reserve((size_t)n + 1))) return rc;
  }

  const size_t n_tiles = (size_t)blocks * (ksplit ? T : 4 * T);  // tiles the screen's waves touch
  if ((rc = sn.xfrag.reserve(n_tiles * 4 * 64))) return rc;
  if ((rc = sn.xstat.reserve(2 * n_tiles * 32))) return rc;
  if ((rc = sn.xok.reserve(n_tiles * 32))) return rc;

  // chunks of the record sort: one record segment per block unless there are too many (the kernels stride then)
  unsigned chunks = (unsigned)n_seg;
  unsigned max_blocks = std::max<unsigned>(2u * g->n_cu, (1u << 20) / (unsigned)g->K);
  if (opt_value(OPT_GMM_SORT_BLOCKS, 0) > 0) max_blocks = (unsigned)opt_value(OPT_GMM_SORT_BLOCKS, 0);
  if (chunks > max_blocks) chunks = max_blocks;
  if ((rc = g->sort.blk_counts.reserve((size_t)chunks * g->K))) return rc;
  const bool kc_lds = g->K <= SCREEN_KC_MAX && !opt_is_set(OPT_GMM_SCREEN_NO_LDS_CONSTS);  // (testing: the global-load path)
  int* const dense_mark = lse ? g->lse.dense_mark.ptr : nullptr;
  int* const dense_count = lse ? reinterpret_cast<int*>(g->lse.dense_list.ptr) : nullptr;  // (in front of the list)

  ProfScope prof(JD_KERNEL_GMM_FWD, s);
  GmmStageArgs stg{};
  set_patch_grid(stg, a);
  stg.flux = a.flux, stg.n_begin = a.n_begin, stg.n_end = a.n_end, stg.n_tiles = (int)n_tiles;
  stg.pcount = lse ? g->lse.pcount.ptr : nullptr, stg.dense_mark = dense_mark, stg.dense_count = dense_count;
  stg.xfrag = sn.xfrag.ptr, stg.xn = sn.xstat.ptr, stg.xs2 = sn.xstat.ptr + n_tiles * 32, stg.ok = sn.xok.ptr, stg.best = sn.best.ptr;
  GmmScreenArgs sc{};
  set_patch_grid(sc, a);
  sc.flux = a.flux, sc.K = a.K, sc.n_begin = a.n_begin, sc.n_end = a.n_end;
  sc.xfrag = sn.xfrag.ptr, sc.xn = stg.xn, sc.xs2 = stg.xs2, sc.ok = sn.xok.ptr;
  sc.afrag16 = sn.afrag16.ptr, sc.const_k = g->dense.const_k.ptr, sc.efro_k = sn.efro_k.ptr, sc.sk2_k = sn.sk2_k.ptr;
  sc.mnorm_k = sn.mnorm_k.ptr, sc.korder = sn.korder.ptr;
  sc.lfinal = sn.lfinal.ptr, sc.rec_n = rec_n, sc.rec_k = rec_k, sc.rec_ub = rec_ub;
  sc.seg_cnt = sn.seg_cnt.ptr, sc.flag = flag, sc.gen = sn.gen, sc.dense_mark = dense_mark;
  {
    ProfScope stage(JD_KERNEL_GMM_STAGE, s);
    gmm_stage_kernel<<<(unsigned)((n_tiles + 3) / 4), 256, 0, s>>>(stg);
  }
  JD_LAUNCH_CHECK();
  {
    ProfScope stage(JD_KERNEL_GMM_SCREEN, s);
    if (lse && ksplit)  // (the caller has checked K <= SCREEN_KC_MAX: the constants table is in LDS)
      gmm_screen_kernel<2, true, true, true><<<blocks, 256, 0, s>>>(sc);
    else if (lse)
      gmm_screen_kernel<2, false, true, true><<<blocks, 256, 0, s>>>(sc);
    else if (ksplit && kc_lds)
      gmm_screen_kernel<2, true, true><<<blocks, 256, 0, s>>>(sc);
    else if (ksplit)
      gmm_screen_kernel<2, true, false><<<blocks, 256, 0, s>>>(sc);
    else if (kc_lds && sn.clock_stamps.ptr) {  // (the default instantiation with the clock stamps: jd_gmm_screen_clock)
      sc.clock_stamps = sn.clock_stamps.ptr, sc.clock_cap = SCREEN_CLOCK_CAP;
      gmm_screen_kernel<2, false, true, false, true><<<blocks, 256, 0, s>>>(sc);
    } else if (kc_lds)
      gmm_screen_kernel<2, false, true><<<blocks, 256, 0, s>>>(sc);
    else
      gmm_screen_kernel<2, false, false><<<blocks, 256, 0, s>>>(sc);
  }
  JD_LAUNCH_CHECK();

  // counting sort of the surviving records by component (the record slot plays the role of the patch index)
  GmmBucketArgs bk{};
  bk.argmax = rec_k, bk.n_begin = 0, bk.n_end = (int)slots, bk.K = g->K;
  bk.counts = sn.ctl.ptr + 1, bk.offsets = sn.ctl.ptr + 1 + 2 * g->K;
  bk.order = sn.rec_order.ptr, bk.order_n = sn.rec_order_n.ptr, bk.gpatch = nullptr;
  bk.seg_cnt = sn.seg_cnt.ptr, bk.seg_cap = SCREEN_CAP, bk.rec_n = rec_n, bk.rec_ub = rec_ub, bk.lfinal = sn.lfinal.ptr;
  bk.chunk = SCREEN_CAP;  // one record segment per chunk
  bk.korder = g->K <= KORDER_MAX_K ? sn.korder.ptr : nullptr;
  if (fused) bk.flag = flag, bk.gen = sn.gen, bk.slot_cap = (int)std::min<size_t>(grec_rows, (size_t)INT32_MAX);
  if (lse) bk.margin = LSE_MARGIN, bk.pcount = g->lse.pcount.ptr, bk.ptab = g->lse.ptab.ptr, bk.ptab_rows = LSE_ROWS, bk.dense_mark = dense_mark;
  bk.blk_counts = g->sort.blk_counts.ptr;
  {
    ProfScope stage(JD_KERNEL_GMM_SORT, s);
    launch_bucket_sort(bk, chunks, s);
  }
  JD_LAUNCH_CHECK();

  GmmExactArgs ex{};
  set_patch_grid(ex, a);
  ex.flux = a.flux, ex.afrag = g->dense.afrag.ptr, ex.mfrag = g->dense.mfrag.ptr, ex.const_k = g->dense.const_k.ptr;
  ex.order_n = sn.rec_order_n.ptr, ex.counts = bk.counts, ex.offsets = bk.offsets, ex.flag = flag, ex.gen = sn.gen;
  ex.gfrag = g->dense.gfrag.ptr, ex.grec = fused ? g->fused.grec.ptr : nullptr, ex.lrec = lse ? g->lse.lrec.ptr : nullptr;
  ex.best = sn.best.ptr, ex.K = g->K;
  if ((rc = launch_exact(g, ex, slots, s))) return rc;

  if (lse) {
    // the dense logsumexp kernel on the groups that hold a marked patch (after a fallback of the pass: on all of them),
    // the records of every other patch -> value and gradient row, the values summed in a fixed order
    GmmBwdLseArgs b{};
    set_patch_grid(b, a);
    b.flux = a.flux, b.afrag = g->dense.afrag.ptr, b.mfrag = g->dense.mfrag.ptr, b.gfrag = g->dense.gfrag.ptr, b.const_k = g->dense.const_k.ptr;
    b.partials = g->dense.partials.ptr, b.gpatch = g->dense.gpatch.ptr, b.K = g->K;
    b.n_begin = a.n_begin, b.n_end = a.n_end, b.run_flag = flag, b.run_gen = sn.gen;
    b.mark = dense_mark, b.vpatch = g->lse.vpatch.ptr;
    b.list = g->lse.dense_list.ptr + 1, b.list_count = dense_count;
    gmm_lse_list_kernel<<<value_blocks, 256, 0, s>>>(dense_mark, a.n_begin, a.n_end, flag, sn.gen, g->lse.dense_list.ptr + 1, dense_count);
    JD_LAUNCH_CHECK();
    long bblocks = ((n + 31) / 32 + 2 * 4 - 1) / (2 * 4);
    if (bblocks > g->n_cu) bblocks = g->n_cu;
    launch_bwd_lse(b, true, (unsigned)bblocks, s);
    JD_LAUNCH_CHECK();
    GmmLseCombineArgs cb{};
    cb.pcount = g->lse.pcount.ptr, cb.ptab = g->lse.ptab.ptr, cb.rows = LSE_ROWS, cb.lrec = g->lse.lrec.ptr, cb.grec = g->fused.grec.ptr;
    cb.gpatch = g->dense.gpatch.ptr, cb.vpatch = g->lse.vpatch.ptr, cb.mark = dense_mark;
    cb.n_begin = a.n_begin, cb.n_end = a.n_end, cb.flag = flag, cb.gen = sn.gen;
    gmm_lse_combine_kernel<<<combine_blocks, 256, 0, s>>>(cb);
    JD_LAUNCH_CHECK();
    gmm_lse_value_kernel<<<value_blocks, 256, 0, s>>>(g->lse.vpatch.ptr, dense_mark, a.n_begin, a.n_end, g->lse.partials.ptr, g->lse.marked.ptr);
    JD_LAUNCH_CHECK();
    gmm_lse_finalize_kernel<<<1, 256, 0, s>>>(g->lse.partials.ptr, g->lse.marked.ptr, (int)value_blocks, flag, sn.gen, value_scale,
                                              value_out, accumulate_value, g->fused.stats.dev, bk.offsets + g->K, (int)n);
    JD_LAUNCH_CHECK();
    *n_partials = 0;
    return JD_OK;
  }

  // fallback: the dense fp32 kernel, gated on the device flag (returns at once in the normal case)
  GmmFwdArgs dense = a;
  dense.run_flag = flag, dense.run_gen = sn.gen, dense.best_out = sn.best.ptr, dense.argmax_out = nullptr, dense.value_patch = nullptr;
  if ((rc = launch_fwd_blocks(MODE_MAX, dense, true, g->n_cu, s, n_partials))) return rc;

  GmmBestArgs be{};
  be.best = sn.best.ptr, be.n_begin = a.n_begin, be.n_end = a.n_end, be.argmax_out = a.argmax_out, be.partials = g->dense.partials.ptr;
  be.flag = flag, be.gen = sn.gen, be.winner = fused ? g->fused.winner.ptr : nullptr, be.argmax_fb = fused ? fallback_argmax : nullptr;
  be.rec_k = rec_k, be.rec_order = sn.rec_order.ptr;
  be.ticket = sn.ctl.ptr + 3 * g->K + 2, be.scale = value_scale, be.value_out = value_out, be.accumulate = accumulate_value;
  be.host_stats = fused ? g->fused.stats.dev : nullptr, be.slots_used = bk.offsets + g->K;
  if (fused) {
    GmmBwdFallbackArgs& b = be.fb;
    set_patch_grid(b, a);
    b.flux = a.flux, b.afrag = g->dense.afrag.ptr, b.mfrag = g->dense.mfrag.ptr, b.gfrag = g->dense.gfrag.ptr;
    b.argmax = fallback_argmax, b.gpatch = g->dense.gpatch.ptr, b.flag = flag, b.gen = sn.gen, b.K = g->K;
    b.n_begin = a.n_begin, b.n_end = a.n_end;
  }
  const unsigned best_blocks = (unsigned)((n + BEST_CHUNK - 1) / BEST_CHUNK);
  gmm_best_kernel<<<best_blocks, 256, 0, s>>>(be);
  JD_LAUNCH_CHECK();
  *n_partials = (int)best_blocks;
  if (opt_is_set(OPT_GMM_SCREEN_DEBUG)) {  // tuning only: synchronises
    std::vector<int> ctl(3 * g->K + 2), seg(n_seg);
    JD_HIP(hipStreamSynchronize(s));
    JD_HIP(hipMemcpy(ctl.data(), sn.ctl.ptr, ctl.size() * sizeof(int), hipMemcpyDeviceToHost));
    JD_HIP(hipMemcpy(seg.data(), sn.seg_cnt.ptr, seg.size() * sizeof(int), hipMemcpyDeviceToHost));
    long survivors = 0, records = 0;
    int seg_max = 0;
    for (int k = 0; k < g->K; ++k) survivors += ctl[1 + k];
    for (int v : seg) records += v, seg_max = v > seg_max ? v : seg_max;
    fprintf(stderr, "[jd gmm screen] patches %ld records %ld (%.2f per patch, fullest wave %d of %d) survivors %ld (%.2f per "
            "patch) fallback %d\n", n, records, (double)records / (double)n, seg_max, SCREEN_CAP, survivors,
            (double)survivors / (double)n, ctl[0] == sn.gen ? 1 : 0);
  }
  return JD_OK;
}

}  // namespace jd

using namespace jd;

// Diagnostics of the screened arg-max path (no synchronisation: whatever pass has landed in the host-mapped block):
// out = {generation of that pass, it fell back to the dense kernel (0 / 1), bucket slots it used, patches it covered,
// gradient rows per patch the record buffer currently has room for}.
extern "C" int jd_gmm_screen_stats(const jd_gmm* g, int* out) {
  JD_REQUIRE(g && out, "jd_gmm_screen_stats: null argument");
  for (int i = 0; i < 4; ++i) out[i] = g->fused.stats.host ? reinterpret_cast<volatile int*>(g->fused.stats.host)[i] : 0;
  out[4] = g->fused.rows_per_patch;
  return JD_OK;
}

// The shader clock INSIDE the screen kernel (round-4 verdict: is the kernel short of its roof, or is the roof lower than the
// nominal clock says?).  First call: allocates the stamp buffer and switches the default screen launch of this handle to
// its stamped instantiation; every later call synchronises the device, averages 100 MHz x (shader ticks / reference
// ticks) over the blocks that have left stamps since the last call, and clears them.
extern "C" int jd_gmm_screen_clock(jd_gmm* g, double* mhz_out, int* samples_out) {
  JD_REQUIRE(g && mhz_out && samples_out, "jd_gmm_screen_clock: null argument");
  JD_REQUIRE(!g->d256, "jd_gmm_screen_clock: D = 256 handles have no screen kernel");
  *mhz_out = 0.0, *samples_out = 0;
  const size_t bytes = (size_t)2 * SCREEN_CLOCK_CAP * sizeof(unsigned long long);
  if (!g->screen.clock_stamps.ptr) {
    if (const int rc = g->screen.clock_stamps.reserve((size_t)2 * SCREEN_CLOCK_CAP)) return rc;
    JD_HIP(hipMemset(g->screen.clock_stamps.ptr, 0, bytes));
    return JD_OK;
  }
  std::vector<unsigned long long> host((size_t)2 * SCREEN_CLOCK_CAP);
  JD_HIP(hipDeviceSynchronize());
  JD_HIP(hipMemcpy(host.data(), g->screen.clock_stamps.ptr, bytes, hipMemcpyDeviceToHost));
  JD_HIP(hipMemset(g->screen.clock_stamps.ptr, 0, bytes));
  double sum = 0.0;
  int n = 0;
  for (int b = 0; b < SCREEN_CLOCK_CAP; ++b)
    if (host[2 * b + 1] > 0) sum += 100.0 * (double)host[2 * b] / (double)host[2 * b + 1], ++n;
  *samples_out = n;
  if (n) *mhz_out = sum / n;
  return JD_OK;
}

// Pyramid of the multi-scale prior (reference: jolideco/priors/patches/core.py:303-324): per level l, f = 2^l,
//   g_l = K_l (*) g_{l-1}   ("same", zero padded, cumulative; K_l = u u^T a sampled Gaussian of `taps` pixels)
//   d_l = f x f mean of g_l (floor: ragged rows / columns dropped)
// and the adjoint of both,
//   dg_{l-1} = K_l^T (*) (dg_l + replicate_f(dd_l) / f^2).
// One launch per level and direction.  A block owns a 32 x 64 tile of the full-resolution image: it stages the tile with
// its halo (taps / 2 <= 21 pixels, zero outside the image) in LDS, runs the row pass and the column pass there, and writes
// the tile from registers.  Tile edges are multiples of 16 and f divides 16, so a pooling cell never straddles two
// blocks: the means are summed inside the block in a fixed order (rows of a cell left to right, then the row sums top to
// bottom) -- no atomics, run-to-run identical.  Loads are unconditional at clamped coordinates through the global address
// space; the zeros of the outside are selected afterwards.
//
// Both kernels are streaming passes, so what a block does per pixel besides the taps has to stay small: a thread keeps
// ONE image column (its lane) and, while staging, one column of the right halo; the four waves of a block take rows in
// turn.  Column coordinates, clamps and rolls are computed once per thread, row coordinates once per row (uniform in a
// wave); nothing divides by a run-time number.  LDS is sized by the launch for the taps it has (18 KB at 3 taps, 50 KB at
// 43), so the narrow blurs of the fine levels keep many blocks on a compute unit.
#include "jd_common.h"
#include "kernels.h"

namespace jd {

constexpr int MS_TH = 32, MS_TW = 64;  // tile (multiples of 16); MS_TW is the wave size: a lane is a column
constexpr int MS_MAX_TAPS = 43;
constexpr int MS_BLOCK = 256, MS_WAVES = MS_BLOCK / 64;
constexpr int MS_KW = 64;              // floats reserved for the taps behind the two images
static_assert(MS_TH % 16 == 0 && MS_TW % 16 == 0, "pooling cells of up to 16 x 16 must not straddle tiles");
static_assert(MS_TW == 64 && MS_TH % (4 * MS_WAVES) == 0, "a lane is a column; a wave takes groups of four rows");

struct MsTaps {
  float w[MS_MAX_TAPS];
};

struct MsValueArgs {  // value_out = sum_i coef[i] * vals[i], in index order, float32 without contraction (the reference's sum)
  const float* vals;
  float* value_out;
  int n;
  float coef[JD_MULTISCALE_MAX_LEVELS];
};

__device__ __forceinline__ void ms_value(const MsValueArgs& v) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (int i = 0; i < v.n; ++i) acc = acc + v.coef[i] * gld(v.vals + i);
  gst(v.value_out, acc);
}

// floats of the staged tile: with pooling the result (TH x TW) and the cells' row sums (<= TH x TW / 2) reuse it
__host__ __device__ inline int ms_tile_floats(int taps, int f) {
  const int staged = (MS_TH + taps - 1) * (MS_TW + taps - 1);
  const int pooled = f > 1 ? MS_TH * MS_TW + MS_TH * MS_TW / 2 : 0;
  return staged > pooled ? staged : pooled;
}
inline size_t ms_lds_bytes(int taps, int f) {
  return sizeof(float) * (size_t)(ms_tile_floats(taps, f) + (MS_TH + taps - 1) * MS_TW + MS_KW);
}

// the taps into LDS, in the order the passes walk them: `flip` = convolution (forward), else correlation (adjoint)
__device__ __forceinline__ void ms_stage_taps(float* kw, const MsTaps& t, int taps, bool flip) {
  float w = 0.f;  // (a chain of selects on constant indices: the struct stays in scalar registers, one LDS store)
#pragma unroll
  for (int i = 0; i < MS_MAX_TAPS; ++i) w = (int)threadIdx.x == i ? t.w[i] : w;
  const int i = threadIdx.x;
  if (i < taps) kw[flip ? taps - 1 - i : i] = w;
}

// Staging: tile[ty][tx] = keep(ty, c) ? load(ty, c) : 0 for the thread's columns tx = lane + 64 c; the waves take rows in
// turn.  The loads of STAGE rows are issued together, before the first of them is stored (one round trip to memory per
// batch, not per row: with 11 a 3-tap tile is one batch, a 43-tap tile two); a row index beyond the tile is clamped for
// the load and not stored.  The adjoint has two loads per element and takes smaller batches (registers).
constexpr int MS_STAGE_DOWN = 11, MS_STAGE_UP = 4;

template <int MS_STAGE, class Load, class Keep>
__device__ __forceinline__ void ms_stage(float* tile, int SW, int rows, Load load, Keep keep) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool second = lane + 64 < SW;
  for (int base = wave; base < rows; base += MS_WAVES * MS_STAGE) {
    float v0[MS_STAGE], v1[MS_STAGE];
#pragma unroll
    for (int s = 0; s < MS_STAGE; ++s) v0[s] = load(min(base + MS_WAVES * s, rows - 1), 0);
    if (second) {
#pragma unroll
      for (int s = 0; s < MS_STAGE; ++s) v1[s] = load(min(base + MS_WAVES * s, rows - 1), 1);
    }
#pragma unroll
    for (int s = 0; s < MS_STAGE; ++s) {
      const int ty = base + MS_WAVES * s;
      if (ty < rows) tile[ty * SW + lane] = keep(ty, 0) ? v0[s] : 0.f;
    }
    if (second) {
#pragma unroll
      for (int s = 0; s < MS_STAGE; ++s) {
        const int ty = base + MS_WAVES * s;
        if (ty < rows) tile[ty * SW + lane + 64] = keep(ty, 1) ? v1[s] : 0.f;
      }
    }
  }
}

// tile[rows x SW] -> mid[rows x TW]:  mid[r][x] = sum_j kw[j] tile[r][x + j].  A thread sums its column for four
// consecutive rows at a time (a tap weight is read once for four sums; lanes walk along x: conflict free).
__device__ __forceinline__ void ms_row_pass(const float* tile, float* mid, const float* kw, int taps, int SW, int rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r0 = 4 * wave; r0 < rows; r0 += 4 * MS_WAVES) {
    const float* p0 = tile + r0 * SW + lane;
    const float* p1 = tile + min(r0 + 1, rows - 1) * SW + lane;  // (the last group may hang over: its extra rows are not stored)
    const float* p2 = tile + min(r0 + 2, rows - 1) * SW + lane;
    const float* p3 = tile + min(r0 + 3, rows - 1) * SW + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < taps; ++k) {
      const float w = kw[k];
      a0 = fmaf(w, p0[k], a0), a1 = fmaf(w, p1[k], a1), a2 = fmaf(w, p2[k], a2), a3 = fmaf(w, p3[k], a3);
    }
    float* m = mid + r0 * MS_TW + lane;
    m[0] = a0;
    if (r0 + 1 < rows) m[MS_TW] = a1;
    if (r0 + 2 < rows) m[2 * MS_TW] = a2;
    if (r0 + 3 < rows) m[3 * MS_TW] = a3;
  }
}

// mid[rows x TW] -> emit(y, acc[4]) for the rows y .. y + 3 of the thread's column:  acc[j] = sum_i kw[i] mid[y + j + i][x],
// from a sliding window (one new value per tap).  Every thread emits TH / 16 groups.
template <class Emit>
__device__ __forceinline__ void ms_col_pass(const float* mid, const float* kw, int taps, Emit emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < MS_TH / (4 * MS_WAVES); ++q) {
    const int y = 4 * (wave + MS_WAVES * q);
    const float* col = mid + y * MS_TW + lane;
    float w0 = col[0], w1 = col[MS_TW], w2 = col[2 * MS_TW];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < taps; ++k) {
      const float w = kw[k];
      const float w3 = col[(k + 3) * MS_TW];  // (row y + k + 3 <= TH - 4 + taps - 1 + 3 = rows - 1)
      acc[0] = fmaf(w, w0, acc[0]), acc[1] = fmaf(w, w1, acc[1]), acc[2] = fmaf(w, w2, acc[2]), acc[3] = fmaf(w, w3, acc[3]);
      w0 = w1, w1 = w2, w2 = w3;
    }
    emit(y, acc);
  }
}

struct MsDownArgs {
  const float* src;  // g_{l-1} (H, W)
  float* g_out;      // g_l (H, W) or null (the last evaluated level: nobody reads it)
  float* d_out;      // d_l (H / f, W / f)
  float* dd_zero;    // dd_l, same shape: zeroed in the same pass (the inner prior accumulates into it), or null
  int H, W, f, log2f, taps;
  int shift_y, shift_x;  // the loads read the image rolled by (shift_y, shift_x), both in [0, H) x [0, W)
};

__global__ __launch_bounds__(MS_BLOCK) void multiscale_down_kernel(MsDownArgs a, MsTaps t) {
  extern __shared__ float ms_lds[];
  const int taps = a.taps, R = taps >> 1, SW = MS_TW + 2 * R, rows = MS_TH + 2 * R;
  float* tile = ms_lds;
  float* mid = tile + ms_tile_floats(taps, a.f);
  float* kw = mid + rows * MS_TW;
  const int lane = threadIdx.x & 63;
  const int y0 = blockIdx.y * MS_TH, x0 = blockIdx.x * MS_TW;
  const int H = a.H, W = a.W;
  ms_stage_taps(kw, t, taps, true);
  {
    // the thread's two columns of the staged tile: lane, and lane + 64 in the right part of the halo (2 R <= 42 columns)
    int xs[2];
    bool xin[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int gx = x0 - R + lane + 64 * c, xc = min(max(gx, 0), W - 1);
      const int x = xc - a.shift_x;  // rolled[y, x] = image[(y - shift_y) mod H, (x - shift_x) mod W]
      xs[c] = x + (x < 0 ? W : 0), xin[c] = gx == xc;
    }
    ms_stage<MS_STAGE_DOWN>(
        tile, SW, rows,
        [&](int ty, int c) {
          const int yc = min(max(y0 - R + ty, 0), H - 1);
          const int y = yc - a.shift_y;
          return gld(a.src + ((size_t)(y + (y < 0 ? H : 0)) * W + xs[c]));
        },
        [&](int ty, int c) {
          const int gy = y0 - R + ty;
          return gy >= 0 && gy < H && xin[c];
        });
  }
  __syncthreads();
  ms_row_pass(tile, mid, kw, taps, SW, rows);
  __syncthreads();  // (every read of `tile` is done: the result may reuse it)
  const int f = a.f, x = x0 + lane;
  float* res = tile;                   // (TH x TW), f > 1 only
  float* part = tile + MS_TH * MS_TW;  // (TH x TW / f) row sums of the cells
  ms_col_pass(mid, kw, taps, [&](int yl, const float* acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + yl + j;
      if (f > 1) res[(yl + j) * MS_TW + lane] = acc[j];
      if (y < H && x < W) {
        const size_t o = (size_t)y * W + x;
        if (a.g_out) gst(a.g_out + o, acc[j]);
        if (f == 1) {
          gst(a.d_out + o, acc[j]);
          if (a.dd_zero) gst(a.dd_zero + o, 0.f);
        }
      }
    }
  });
  if (f == 1) return;  // (uniform)
  __syncthreads();
  const int lf = a.log2f, lcw = 6 - lf, cw = MS_TW >> lf, ch = MS_TH >> lf;
  const int Hp = H >> lf, Wp = W >> lf;
  for (int i = threadIdx.x; i < MS_TH * cw; i += MS_BLOCK) {
    const int y = i >> lcw, cx = i & (cw - 1);
    const float* p = res + y * MS_TW + (cx << lf);
    float s = 0.f;
    for (int j = 0; j < f; ++j) s += p[j];
    part[i] = s;
  }
  __syncthreads();
  const float inv = 1.f / (float)(f * f);
  for (int i = threadIdx.x; i < ch * cw; i += MS_BLOCK) {
    const int cy = i >> lcw, cx = i & (cw - 1);
    const float* p = part + ((cy << lf) << lcw) + cx;
    float s = 0.f;
    for (int j = 0; j < f; ++j) s += p[j << lcw];
    const int py = (y0 >> lf) + cy, px = (x0 >> lf) + cx;
    if (py < Hp && px < Wp) {  // (a whole cell inside the image: the ragged ones are dropped)
      const size_t o = (size_t)py * Wp + px;
      gst(a.d_out + o, s * inv);
      if (a.dd_zero) gst(a.dd_zero + o, 0.f);
    }
  }
}

struct MsUpArgs {
  const float* dg;   // dg_l (H, W) or null
  const float* dd;   // dd_l (H / f, W / f)
  float* out;        // dg_{l-1} (H, W): assigned; or, with `rolled`, the gradient image: out[(y - sy) mod H, (x - sx) mod W] += .
  int H, W, f, log2f, taps;
  int rolled, shift_y, shift_x;
};

__global__ __launch_bounds__(MS_BLOCK) void multiscale_up_kernel(MsUpArgs a, MsTaps t, MsValueArgs v) {
  extern __shared__ float ms_lds[];
  const int taps = a.taps, R = taps >> 1, SW = MS_TW + 2 * R, rows = MS_TH + 2 * R;
  float* tile = ms_lds;
  float* mid = tile + ms_tile_floats(taps, 1);
  float* kw = mid + rows * MS_TW;
  const int lane = threadIdx.x & 63;
  const int y0 = blockIdx.y * MS_TH, x0 = blockIdx.x * MS_TW;
  const int H = a.H, W = a.W, lf = a.log2f;
  const int Hp = H >> lf, Wp = W >> lf;
  const float inv = 1.f / (float)(a.f * a.f);
  const bool has_dg = a.dg != nullptr;
  ms_stage_taps(kw, t, taps, false);
  {
    int xc[2], px[2];
    bool xin[2], pin[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int gx = x0 - R + lane + 64 * c;
      xc[c] = min(max(gx, 0), W - 1), xin[c] = gx == xc[c];
      const int p = xc[c] >> lf;  // the pooling cell of the column, clamped into the pooled image
      pin[c] = p < Wp, px[c] = min(p, Wp - 1);
    }
    ms_stage<MS_STAGE_UP>(
        tile, SW, rows,
        [&](int ty, int c) {
          const int yc = min(max(y0 - R + ty, 0), H - 1);
          const int py = yc >> lf;
          float s = gld(a.dd + ((size_t)min(py, Hp - 1) * Wp + px[c])) * inv;
          s = (py < Hp && pin[c]) ? s : 0.f;
          if (has_dg) s += gld(a.dg + ((size_t)yc * W + xc[c]));
          return s;
        },
        [&](int ty, int c) {
          const int gy = y0 - R + ty;
          return gy >= 0 && gy < H && xin[c];
        });
  }
  __syncthreads();
  ms_row_pass(tile, mid, kw, taps, SW, rows);
  __syncthreads();
  const int x = x0 + lane;
  int xr = x - a.shift_x;
  xr += xr < 0 ? W : 0;
  ms_col_pass(mid, kw, taps, [&](int yl, const float* acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + yl + j;
      if (y < H && x < W) {
        if (a.rolled) {
          int yr = y - a.shift_y;
          yr += yr < 0 ? H : 0;
          float* p = a.out + ((size_t)yr * W + xr);
          gst(p, gld(p) + acc[j]);  // (every pixel of the gradient image belongs to one thread of one block)
        } else {
          gst(a.out + ((size_t)y * W + x), acc[j]);
        }
      }
    }
  });
  if (v.value_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ms_value(v);
}

__global__ void multiscale_value_kernel(MsValueArgs v) {
  if (threadIdx.x == 0) ms_value(v);
}

static int ms_check(const char* who, int H, int W, int f, const float* taps, int n_taps) {
  JD_REQUIRE(taps, "%s: null argument", who);
  JD_REQUIRE(f == 1 || f == 2 || f == 4 || f == 8 || f == 16, "%s: pooling factor %d not in {1, 2, 4, 8, 16}", who, f);
  JD_REQUIRE(n_taps >= 1 && n_taps <= MS_MAX_TAPS && n_taps % 2 == 1, "%s: %d taps: an odd number of at most %d is supported", who,
             n_taps, MS_MAX_TAPS);
  JD_REQUIRE(H >= f && W >= f, "%s: image %d x %d smaller than the pooling factor %d", who, H, W, f);
  JD_REQUIRE((long long)H * W < (1ll << 31), "%s: image %d x %d too large", who, H, W);
  return JD_OK;
}

static int ms_log2(int f) {
  int lf = 0;
  while ((1 << lf) < f) ++lf;
  return lf;
}

static int ms_value_args(const char* who, MsValueArgs& v, const float* vals, const float* coefs, int n, float* value_out) {
  v.vals = vals, v.value_out = value_out, v.n = 0;
  if (!value_out) return JD_OK;
  JD_REQUIRE(vals && coefs, "%s: null argument (level values / coefficients with value_out)", who);
  JD_REQUIRE(n >= 1 && n <= JD_MULTISCALE_MAX_LEVELS, "%s: %d level values not in [1, %d]", who, n, JD_MULTISCALE_MAX_LEVELS);
  v.n = n;
  for (int i = 0; i < n; ++i) v.coef[i] = coefs[i];
  return JD_OK;
}

static dim3 ms_grid(int H, int W) { return dim3((unsigned)((W + MS_TW - 1) / MS_TW), (unsigned)((H + MS_TH - 1) / MS_TH)); }

}  // namespace jd

using namespace jd;

extern "C" int jd_multiscale_down(const float* src, int H, int W, int f, const float* taps, int n_taps, int shift_y, int shift_x,
                                  float* g_out, float* d_out, float* dd_zero, void* stream) {
  JD_REQUIRE(src && d_out, "jd_multiscale_down: null argument");
  int rc = ms_check("jd_multiscale_down", H, W, f, taps, n_taps);
  if (rc) return rc;
  JD_REQUIRE(shift_y >= 0 && shift_y < H && shift_x >= 0 && shift_x < W, "jd_multiscale_down: roll (%d, %d) not reduced modulo the shape %d x %d",
             shift_y, shift_x, H, W);
  JD_REQUIRE(g_out != src, "jd_multiscale_down: g_out must not alias src (blocks read their neighbours' pixels)");
  MsDownArgs a{src, g_out, d_out, dd_zero, H, W, f, ms_log2(f), n_taps, shift_y, shift_x};
  MsTaps t{};
  for (int i = 0; i < n_taps; ++i) t.w[i] = taps[i];
  hipStream_t s = as_stream(stream);
  {
    ProfScope prof(JD_KERNEL_MULTISCALE_DOWN, s);
    multiscale_down_kernel<<<ms_grid(H, W), MS_BLOCK, ms_lds_bytes(n_taps, f), s>>>(a, t);
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}

extern "C" int jd_multiscale_up_adjoint(const float* dg, const float* dd, int H, int W, int f, const float* taps, int n_taps,
                                        float* out, int rolled, int shift_y, int shift_x, const float* level_values,
                                        const float* level_coefs, int n_values, float* value_out, void* stream) {
  JD_REQUIRE(dd && out, "jd_multiscale_up_adjoint: null argument");
  int rc = ms_check("jd_multiscale_up_adjoint", H, W, f, taps, n_taps);
  if (rc) return rc;
  JD_REQUIRE(shift_y >= 0 && shift_y < H && shift_x >= 0 && shift_x < W,
             "jd_multiscale_up_adjoint: roll (%d, %d) not reduced modulo the shape %d x %d", shift_y, shift_x, H, W);
  JD_REQUIRE(rolled || (shift_y == 0 && shift_x == 0), "jd_multiscale_up_adjoint: a roll needs the accumulating form (rolled = 1)");
  JD_REQUIRE(out != dg, "jd_multiscale_up_adjoint: out must not alias dg (blocks read their neighbours' pixels)");
  MsValueArgs v{};
  if ((rc = ms_value_args("jd_multiscale_up_adjoint", v, level_values, level_coefs, n_values, value_out))) return rc;
  MsUpArgs a{dg, dd, out, H, W, f, ms_log2(f), n_taps, rolled ? 1 : 0, shift_y, shift_x};
  MsTaps t{};
  for (int i = 0; i < n_taps; ++i) t.w[i] = taps[i];
  hipStream_t s = as_stream(stream);
  {
    ProfScope prof(JD_KERNEL_MULTISCALE_UP, s);
    multiscale_up_kernel<<<ms_grid(H, W), MS_BLOCK, ms_lds_bytes(n_taps, 1), s>>>(a, t, v);
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}

extern "C" int jd_multiscale_value(const float* level_values, const float* level_coefs, int n_values, float* value_out,
                                   void* stream) {
  JD_REQUIRE(value_out, "jd_multiscale_value: null argument");
  MsValueArgs v{};
  int rc = ms_value_args("jd_multiscale_value", v, level_values, level_coefs, n_values, value_out);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  multiscale_value_kernel<<<1, 64, 0, s>>>(v);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

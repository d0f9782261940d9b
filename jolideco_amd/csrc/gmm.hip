// GMM patch prior for 8x8 patches on gfx950 (CDNA4): the handle and the public entries.  The kernels live in
// gmm_dense.hip (dense forward and backward, where the method is described), gmm_sort.hip (counting sort),
// gmm_screen.hip (screened arg-max / logsumexp) and gmm_gather.hip (image norm, overlap-add, band sums); 16x16 patches
// in gmm256.hip.
#include <memory>

#include "gmm_internal.h"

using namespace jd;

extern "C" int jd_gmm_create(int K, int Dn, const float* prec_chol, const float* mu_prec, const float* const_k,
                             const float* pixel_w, jd_gmm** gmm_out) {
  JD_REQUIRE(gmm_out && prec_chol && mu_prec && const_k && pixel_w, "jd_gmm_create: null argument");
  JD_REQUIRE(K >= 1 && K <= BUCKET_MAX_K, "jd_gmm_create: K = %d out of range [1, %d]", K, BUCKET_MAX_K);
  JD_REQUIRE(Dn == D || Dn == 256, "jd_gmm_create: only 8x8 and 16x16 patches (D = 64 or D = 256) are supported, got D = %d", Dn);
  std::unique_ptr<jd_gmm> g(new (std::nothrow) jd_gmm());  // (owns every allocation below: an early return frees them)
  if (!g) return fail(JD_ERR_ALLOC, "jd_gmm_create: out of host memory");
  g->K = K;
  if (Dn == 256) {
    if (const int rc256 = gmm256_create(K, prec_chol, mu_prec, const_k, pixel_w, &g->d256)) return rc256;
    *gmm_out = g.release();
    return JD_OK;
  }

  std::vector<float> afrag((size_t)K * AFRAG_FLOATS), gfrag((size_t)K * AFRAG_FLOATS), mfrag((size_t)K * 64),
      prow((size_t)D * D), mrow(D);
  double sw[D];
  for (int j = 0; j < D; ++j) sw[j] = std::sqrt((double)pixel_w[j]);
  bool tri = true;
  for (int k = 0; k < K; ++k) {
    const float* Pk = prec_chol + (size_t)k * D * D;
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) {
        prow[(size_t)i * D + j] = (float)((double)Pk[i * D + j] * sw[j]);  // P'[i][j] = P[i][j] * sqrt(w_j)
        if (i > j && Pk[i * D + j] != 0.f) tri = false;
      }
    for (int j = 0; j < D; ++j) mrow[j] = (float)((double)mu_prec[(size_t)k * D + j] * sw[j]);
    // forward A fragments [jb][st4][lane][e]: P'[pixel 16 st4 + 4 e + (lane >> 4)][16 jb + (lane & 15)]
    for (int jb = 0; jb < 4; ++jb)
      for (int st4 = 0; st4 < 4; ++st4)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e) {
            const int pix = 16 * st4 + 4 * e + (lane >> 4), j = 16 * jb + (lane & 15);
            afrag[(size_t)k * AFRAG_FLOATS + (((jb * 4 + st4) * 64 + lane) * 4 + e)] = prow[(size_t)pix * D + j];
          }
    // backward A fragments [ib][jb][lane][r]: P'[16 ib + (lane & 15)][16 jb + 4 (lane >> 4) + r]
    for (int ib = 0; ib < 4; ++ib)
      for (int jb = 0; jb < 4; ++jb)
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 4; ++r) {
            const int pix = 16 * ib + (lane & 15), j = 16 * jb + 4 * (lane >> 4) + r;
            gfrag[(size_t)k * AFRAG_FLOATS + (((ib * 4 + jb) * 64 + lane) * 4 + r)] = prow[(size_t)pix * D + j];
          }
    // accumulator init [jb][g][r] = -m'[16 jb + 4 g + r]
    for (int j = 0; j < D; ++j) mfrag[(size_t)k * 64 + j] = -mrow[j];
  }
  g->triangular = tri;
  // screening operands: fp16(P' / s_k) in 32x32x16 A-fragment order, blocks (jb, s) = (0,0) (0,1) (1,0) (1,1) (1,2) (1,3):
  // lane l holds A[row l & 31][k = 8 (l >> 5) + e] = P'[pixel 16 s + 8 (l >> 5) + e][32 jb + (l & 31)]
  bool screenable = true;
  std::vector<uint16_t> a16;
  std::vector<float> efro, sk2, mnorm;
  if (tri) {
    auto to_half = [](float f) -> uint16_t {  // IEEE binary16, round to nearest even (|f| < 65504 here)
      uint32_t u;
      memcpy(&u, &f, 4);
      const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
      const int32_t e = (int32_t)((u >> 23) & 0xFF) - 127;
      uint32_t m = u & 0x7FFFFFu;
      if (e < -25) return sign;               // underflows to zero
      if (e < -14) {                          // subnormal half
        m |= 0x800000u;
        const int shift = -e - 14 + 13;       // 14 .. 24
        uint32_t h = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (h & 1u))) ++h;
        return (uint16_t)(sign | h);
      }
      uint32_t h = ((uint32_t)(e + 15) << 10) | (m >> 13);
      const uint32_t rem = m & 0x1FFFu;
      if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;  // a carry into the exponent is the right answer
      return (uint16_t)(sign | h);
    };
    static const int blk_jb[A16_BLOCKS] = {0, 0, 1, 1, 1, 1}, blk_s[A16_BLOCKS] = {0, 1, 0, 1, 2, 3};
    a16.resize((size_t)K * A16_BLOCKS * 64 * 8);
    efro.resize(K);
    sk2.resize(K);
    mnorm.resize(K);
    for (int k = 0; k < K; ++k) {
      const float* Pk = prec_chol + (size_t)k * D * D;
      double fro = 0.0, amax = 0.0;
      for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
          const float v = (float)((double)Pk[i * D + j] * sw[j]);
          fro += (double)v * v;
          amax = std::fmax(amax, std::fabs((double)v));
        }
      // fp16 operand P'_k / s_k with the power of two s_k that puts max |P'_k| into [2^13, 2^14)
      int ex = 14;
      if (amax > 0.0 && std::isfinite(amax)) (void)std::frexp(amax, &ex);
      const double inv_s = std::ldexp(1.0, 14 - ex);
      sk2[k] = (float)std::ldexp(1.0, 2 * (ex - 14));
      efro[k] = (float)(std::sqrt(fro) * (double)SCREEN_EPS * 1.0011);  // includes the 1.001 inflation of the bound
      double m2 = 0.0;
      for (int j = 0; j < D; ++j) {
        const double m = (double)mu_prec[(size_t)k * D + j] * sw[j];
        m2 += m * m;
      }
      mnorm[k] = (float)(std::sqrt(m2) * 1.0011);
      if (!std::isfinite(efro[k]) || !std::isfinite(mnorm[k]) || !(sk2[k] > 0.f) || !std::isfinite(sk2[k])) screenable = false;
      for (int b = 0; b < A16_BLOCKS; ++b)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e) {
            const int pix = 16 * blk_s[b] + 8 * (lane >> 5) + e, j = 32 * blk_jb[b] + (lane & 31);
            const float v = (float)((double)Pk[pix * D + j] * sw[j] * inv_s);
            a16[(((size_t)k * A16_BLOCKS + b) * 64 + lane) * 8 + e] = to_half(v);
          }
    }
    if (!screenable) a16.clear();
  }
  auto upload = [&](DevBuf<float>& dst, const float* src, size_t n) -> int {
    if (const int rc = dst.reserve(n)) return rc;
    JD_HIP(hipMemcpy(dst.ptr, src, n * sizeof(float), hipMemcpyHostToDevice));
    return JD_OK;
  };
  int rc;
  if ((rc = upload(g->dense.afrag, afrag.data(), afrag.size())) || (rc = upload(g->dense.mfrag, mfrag.data(), mfrag.size())) ||
      (rc = g->dense.const_k.reserve(2 * (size_t)K)) || (rc = upload(g->dense.const_k, const_k, K)) || (rc = upload(g->dense.gfrag, gfrag.data(), gfrag.size())))
    return rc;
  JD_HIP(hipMemset(g->dense.const_k.ptr + K, 0, (size_t)K * sizeof(float)));  // (the residuals of c_k: zero until set)
  if (g->sort.bucket.reserve((size_t)(3 * K + 1)) || hipMemset(g->sort.bucket.ptr, 0, (size_t)(3 * K + 1) * sizeof(int)) != hipSuccess)
    return fail(JD_ERR_ALLOC, "jd_gmm_create: hipMalloc of the bucket counters failed");
  if (!a16.empty()) {
    jd_gmm::Screen& sn = g->screen;
    if (sn.afrag16.reserve(a16.size() / 8) ||  // (8 fp16 per uint4)
        hipMemcpy(sn.afrag16.ptr, a16.data(), a16.size() * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess ||
        (rc = upload(sn.efro_k, efro.data(), efro.size())) || (rc = upload(sn.sk2_k, sk2.data(), sk2.size())) ||
        (rc = upload(sn.mnorm_k, mnorm.data(), mnorm.size())) || sn.ctl.reserve((size_t)(3 * K + 3)) ||
        hipMemset(sn.ctl.ptr, 0, (size_t)(3 * K + 3) * sizeof(int)) != hipSuccess || sn.korder.reserve((size_t)K))
      return fail(JD_ERR_ALLOC, "jd_gmm_create: allocation of the screening operands failed");
    std::vector<int> identity(K);
    for (int k = 0; k < K; ++k) identity[k] = k;
    if (hipMemcpy(sn.korder.ptr, identity.data(), (size_t)K * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
      return fail(JD_ERR_HIP, "jd_gmm_create: upload of the component order failed");
    sn.ok = true;
    // statistics of the last finished pass in host-mapped memory (optional: without it the record buffer keeps its
    // initial capacity)
    MappedStats& st = g->fused.stats;
    void* mapped = nullptr;
    if (!opt_is_set(OPT_GMM_NO_HOST_STATS) &&
        hipHostMalloc(reinterpret_cast<void**>(&st.host), 4 * sizeof(int), hipHostMallocMapped) == hipSuccess) {
      memset(st.host, 0, 4 * sizeof(int));
      if (hipHostGetDevicePointer(&mapped, st.host, 0) == hipSuccess) {
        st.dev = static_cast<int*>(mapped);
      } else {
        (void)hipHostFree(st.host);
        st.host = nullptr;
      }
    } else {
      st.host = nullptr;
    }
  }
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
    g->n_cu = prop.multiProcessorCount;
  *gmm_out = g.release();
  return JD_OK;
}

extern "C" int jd_gmm_destroy(jd_gmm* g) {
  if (!g) return JD_OK;
  (void)hipDeviceSynchronize();
  if (g->d256) gmm256_destroy(g->d256);
  delete g;  // (every device array of the handle is a DevBuf)
  return JD_OK;
}

extern "C" int jd_gmm_is_triangular(const jd_gmm* g) {
  if (g && g->d256) return gmm256_is_triangular(g->d256) ? 1 : 0;
  return g ? (g->triangular ? 1 : 0) : -1;
}

// The image norm the following jd_gmm_prior_* calls of this handle apply (header: jd_image_norm).
extern "C" int jd_gmm_set_image_norm(jd_gmm* g, const jd_image_norm* norm) {
  JD_REQUIRE(norm, "jd_gmm_set_image_norm: null argument");
  JD_REQUIRE(norm->kind >= 0 && norm->kind < NORM_COUNT, "jd_gmm_set_image_norm: unknown image norm kind %d", norm->kind);
  if (norm->kind != NORM_IDENTITY) {
    // every norm divides by a scale (asinh, sigmoid, atan, log: alpha = p0; fixed-max: max_value = p0; power: beta = p1)
    const float scale = norm->kind == NORM_POWER ? norm->p1 : norm->p0;
    JD_REQUIRE(std::isfinite(norm->p0) && std::isfinite(norm->p1), "jd_gmm_set_image_norm: non-finite parameter (%g, %g) of image norm kind %d",
               (double)norm->p0, (double)norm->p1, norm->kind);
    JD_REQUIRE(scale != 0.f, "jd_gmm_set_image_norm: image norm kind %d divides by its scale parameter, which is 0", norm->kind);
    JD_REQUIRE(norm->kind != NORM_ASINH || norm->p1 != 0.f, "jd_gmm_set_image_norm: asinh norm with beta = 0 (asinh(beta / alpha) = 0 divides)");
  }
  JD_REQUIRE(g, "jd_gmm_set_image_norm: null argument");
  ImageNormArgs nm{};
  nm.kind = norm->kind;
  if (nm.kind != NORM_IDENTITY) nm.p0 = norm->p0, nm.p1 = norm->p1;
  if (nm.kind == NORM_ASINH) nm.c = std::asinh(nm.p1 / nm.p0);
  g->norm = nm;
  return JD_OK;
}

// The patch norm the following jd_gmm_prior_* calls of this handle apply (header: jd_gmm_set_patch_norm).
extern "C" int jd_gmm_set_patch_norm(jd_gmm* g, int kind) {
  JD_REQUIRE(kind >= 0 && kind < PATCH_NORM_COUNT, "jd_gmm_set_patch_norm: unknown patch norm kind %d", kind);
  JD_REQUIRE(g, "jd_gmm_set_patch_norm: null argument");
  g->patch_norm = kind;
  return JD_OK;
}

// The part of c_k a float32 const_k cannot hold (header: jd_gmm_set_const_residual): the second half of the constants' array.
extern "C" int jd_gmm_set_const_residual(jd_gmm* g, const float* residual) {
  JD_REQUIRE(g && residual, "jd_gmm_set_const_residual: null argument");
  for (int k = 0; k < g->K; ++k)
    JD_REQUIRE(std::isfinite(residual[k]), "jd_gmm_set_const_residual: residual[%d] is not finite", k);
  if (g->d256) return gmm256_set_const_residual(g->d256, residual);
  JD_HIP(hipDeviceSynchronize());  // (no pass of this handle is reading the constants)
  JD_HIP(hipMemcpy(g->dense.const_k.ptr + g->K, residual, (size_t)g->K * sizeof(float), hipMemcpyHostToDevice));
  return JD_OK;
}

// Backward pass of the arg-max mode without the screen's fused rows: the patches are bucketed by their arg-max component
// (`arg`), then one wave per 32 patches that share P'_k (gmm_bwd_max_kernel) -> g->dense.gpatch.
static int bucketed_backward(jd_gmm* g, const float* flux, const PatchGrid& grid, int n_begin, int n_end, const int32_t* arg,
                             hipStream_t s, int patch_norm) {
  const long n = n_end - n_begin;
  int rc;
  const size_t slots_cap = (size_t)n + 32 * (size_t)g->K;
  if ((rc = g->sort.order.reserve(slots_cap))) return rc;
  GmmBucketArgs bk{};
  bk.argmax = arg, bk.n_begin = n_begin, bk.n_end = n_end, bk.K = g->K;
  bk.counts = g->sort.bucket.ptr, bk.offsets = g->sort.bucket.ptr + 2 * g->K;
  bk.order = g->sort.order.ptr, bk.gpatch = g->dense.gpatch.ptr;
  bk.chunk = BUCKET_CHUNK;
  unsigned chunks = (unsigned)((n + BUCKET_CHUNK - 1) / BUCKET_CHUNK);
  const unsigned max_blocks = std::max<unsigned>(2u * g->n_cu, (1u << 20) / (unsigned)g->K);
  if (chunks > max_blocks) chunks = max_blocks;
  if ((rc = g->sort.blk_counts.reserve((size_t)chunks * g->K))) return rc;
  bk.blk_counts = g->sort.blk_counts.ptr;
  {
    ProfScope prof(JD_KERNEL_GMM_BWD, s);
    launch_bucket_sort(bk, chunks, s);
    GmmBwdArgs b{};
    set_patch_grid(b, grid);
    b.flux = flux, b.afrag = g->dense.afrag.ptr, b.mfrag = g->dense.mfrag.ptr, b.gfrag = g->dense.gfrag.ptr, b.argmax = arg;
    b.order = g->sort.order.ptr, b.offsets = bk.offsets, b.counts = bk.counts, b.gpatch = g->dense.gpatch.ptr, b.K = g->K;
    b.n_begin = n_begin, b.n_end = n_end;
    long bwd_blocks = ((long)(slots_cap / 32) + 3) / 4;
    const long cap = (long)g->n_cu * 3;  // 3 blocks of 4 waves per CU: one wave per SIMD x 3
    if (bwd_blocks > cap) bwd_blocks = cap;
    launch_bwd_max(b, g->triangular && !opt_is_set(OPT_GMM_DENSE), (unsigned)bwd_blocks, s, patch_norm);
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}

static int gmm_prior_impl(jd_gmm* g, const ImageNormArgs& norm, const float* flux, int H, int W, int stride, int shift_y,
                          int shift_x, int patch_row_begin, int patch_row_end, int marginalize,
                          float value_scale, float* value_out, int accumulate_value, float grad_coef,
                          float* grad_flux_accum, int32_t* argmax_out, float* band_out, void* stream,
                          const AdamArgs* step = nullptr, const int* shift_dev = nullptr, int phases = 3) {
  JD_REQUIRE(g && flux && value_out, "jd_gmm_prior_fwd_bwd: null argument");
  JD_REQUIRE(phases >= 1 && phases <= 3, "jd_gmm_prior_fwd_bwd: phases = %d not in [1, 3]", phases);
  JD_REQUIRE(H >= P && W >= P, "jd_gmm_prior_fwd_bwd: image (%d, %d) smaller than a patch", H, W);
  JD_REQUIRE(stride >= 1 && stride <= P, "jd_gmm_prior_fwd_bwd: stride = %d not in [1, 8]", stride);
  const int nPy = (H - P) / stride + 1, nPx = (W - P) / stride + 1;
  JD_REQUIRE((long)nPy * nPx < (1L << 31), "jd_gmm_prior_fwd_bwd: too many patches");
  if (patch_row_end < 0) patch_row_end = nPy;
  JD_REQUIRE(patch_row_begin >= 0 && patch_row_begin <= patch_row_end && patch_row_end <= nPy,
             "jd_gmm_prior_fwd_bwd: patch row range [%d, %d) outside [0, %d]", patch_row_begin, patch_row_end, nPy);
  hipStream_t s = as_stream(stream);
  shift_y = roll_residue(shift_y, H), shift_x = roll_residue(shift_x, W);
  const int n_begin = patch_row_begin * nPx, n_end = patch_row_end * nPx;
  if (n_begin == n_end) {  // empty shard: contributes nothing (an empty band has no rows)
    if (!accumulate_value) JD_HIP(hipMemsetAsync(value_out, 0, sizeof(float), s));
    return JD_OK;
  }
  if (band_out) grad_flux_accum = band_out;  // "a gradient is wanted"; the gather writes the band instead
  if (step) {
    JD_REQUIRE(!band_out && patch_row_begin == 0 && patch_row_end == nPy && stride >= 4 && opt_value(OPT_GMM_GATHER_TILED, 1) != 0,
               "jd_gmm_prior_fwd_bwd_step: needs the whole prior (no shard, no band) and stride >= 4");
    grad_flux_accum = step->grad_flux;  // "a gradient is wanted"; the gather reads it and applies the step instead
  }
  const long n = n_end - n_begin;
  const PatchGrid grid{H, W, stride, nPx, shift_y, shift_x, shift_dev};
  int rc;
  // phases: bit 0 = everything up to the per-patch gradient rows (value, arg-max, rows: reads the flux only), bit 1 = the
  // gather (+ optimizer step) of those rows into the gradient image.  Called with 1 and later with 2 -- the same arguments --
  // the two halves may sit on different streams: the caller runs the first beside the likelihood launches of the step (it
  // does not touch the gradient image) and joins the streams in front of the second (jolideco_amd/core.py).
  bool screened = false, fused = false, lse_screened = false;
  const bool has_norm = norm.kind != NORM_IDENTITY;
  // The standardized patch norm takes the dense kernels only: the screen's error bounds are those of mean-free patches.
  const int patch_norm = g->patch_norm;
  const bool screenable = patch_norm == PATCH_NORM_SUBTRACT_MEAN;
  const float* const raw_flux = flux;
  if (phases & 1) {
    if (has_norm) {  // everything below reads n(flux); it still only READS the flux (legal beside the likelihood)
      if ((rc = g->normed.reserve((size_t)H * W))) return rc;
      if ((rc = launch_image_norm(raw_flux, g->normed.ptr, (size_t)H * W, norm, g->n_cu, s))) return rc;
      flux = g->normed.ptr;
    }
    if ((rc = g->dense.partials.reserve((size_t)((n + 31) / 32 + 4)))) return rc;
    // option JD_GMM_SCREEN = 0 forces the dense fp32 kernel (testing / tuning)
    screened = screenable && !marginalize && g->screen.ok && opt_value(OPT_GMM_SCREEN, 1) != 0 && !opt_is_set(OPT_GMM_DENSE);
    // screened arg-max with a gradient: the exact kernel also produces the gradient rows (no second sort, no separate
    // backward kernel); JD_GMM_FUSED_BWD=0 keeps the bucketed backward pass (testing / tuning)
    fused = screened && grad_flux_accum && g->triangular && opt_value(OPT_GMM_FUSED_BWD, 1) != 0;
    // logsumexp mode with a gradient: through the screen as well (option JD_GMM_LSE_SCREEN = 0: the dense kernels)
    lse_screened = screenable && marginalize && grad_flux_accum && g->screen.ok && g->triangular && g->K <= SCREEN_KC_MAX &&
                        opt_value(OPT_GMM_LSE_SCREEN, 1) != 0 && !opt_is_set(OPT_GMM_DENSE);
    if (lse_screened && g->fused.stats.host && opt_value(OPT_GMM_LSE_SCREEN, 1) != 2) {  // (2: always, for tests and timing)
      volatile int* hs = g->fused.stats.host;
      const int seen = hs[0];
      if (g->lse.last_pass && seen == g->screen.gen && seen != g->lse.seen_gen) {  // the previous pass has landed and was screened
        g->lse.seen_gen = seen;
        if (hs[1] == 2 || (hs[1] == 1 && g->fused.rows_per_patch >= 32)) g->lse.skip = 32;
      }
      if (g->lse.skip > 0) --g->lse.skip, lse_screened = false;
    }
    g->lse.last_pass = lse_screened;
    int32_t* arg = argmax_out;
    if (grad_flux_accum && (!arg || fused)) {  // fused: the internal buffer holds the components after a fallback
      if ((rc = g->dense.argmax.reserve((size_t)nPy * nPx))) return rc;
      if (!arg) arg = g->dense.argmax.ptr;
    }
    GmmFwdArgs a{};
    set_patch_grid(a, grid);
    a.flux = flux, a.afrag = g->dense.afrag.ptr, a.mfrag = g->dense.mfrag.ptr, a.const_k = g->dense.const_k.ptr, a.K = g->K;
    a.n_begin = n_begin, a.n_end = n_end, a.argmax_out = fused ? argmax_out : arg, a.value_patch = nullptr, a.partials = g->dense.partials.ptr;
    if (grad_flux_accum && (rc = g->dense.gpatch.reserve((size_t)n * D))) return rc;  // (the fused fallback writes it)
    int n_waves = 0;
    if (lse_screened)
      rc = screened_forward(g, a, s, &n_waves, true, nullptr, (double)value_scale, value_out, accumulate_value, true);
    else if (marginalize && grad_flux_accum) {
      // value and gradient rows in one pass over the components (gmm_bwd_lse_kernel)
      GmmBwdLseArgs b{};
      set_patch_grid(b, grid);
      b.flux = flux, b.afrag = g->dense.afrag.ptr, b.mfrag = g->dense.mfrag.ptr, b.gfrag = g->dense.gfrag.ptr, b.const_k = g->dense.const_k.ptr;
      b.gpatch = g->dense.gpatch.ptr, b.K = g->K, b.n_begin = n_begin, b.n_end = n_end;
      const long groups = (n + 31) / 32;
      long blocks = (groups + 2 * 4 - 1) / (2 * 4);  // 2 groups per wave, 4 waves per block
      if (blocks > g->n_cu) blocks = g->n_cu;       // one block per CU (one wave per SIMD), grid-stride over the rest
      if ((rc = g->dense.partials.reserve((size_t)blocks))) return rc;
      b.partials = g->dense.partials.ptr;
      n_waves = (int)blocks;
      ProfScope prof(JD_KERNEL_GMM_BWD, s);
      launch_bwd_lse(b, g->triangular && !opt_is_set(OPT_GMM_DENSE), (unsigned)blocks, s, patch_norm);
      JD_LAUNCH_CHECK();
    } else if (marginalize)
      rc = launch_fwd(MODE_LSE, a, g->triangular, g->n_cu, s, &n_waves, patch_norm);
    else if (screened)
      rc = screened_forward(g, a, s, &n_waves, fused, fused ? g->dense.argmax.ptr : nullptr, (double)value_scale, value_out, accumulate_value);
    else
      rc = launch_fwd(MODE_MAX, a, g->triangular, g->n_cu, s, &n_waves, patch_norm);
    if (rc) return rc;
    // (screened path: the last block of gmm_best_kernel has written the value already)
    if (!screened && !lse_screened &&
        (rc = launch_finalize_sum(g->dense.partials.ptr, n_waves, (double)value_scale, 0.0, value_out, accumulate_value, s)))
      return rc;
    if (!grad_flux_accum) return JD_OK;

    if ((rc = g->dense.gpatch.reserve((size_t)n * D))) return rc;
    // lse_screened: the combine kernel (or, after a fallback, the gated dense backward kernel) has written g->dense.gpatch;
    // marginalize: gmm_bwd_lse_kernel has written the rows together with the value; fused: the rows are in g->fused.grec
    // already (after a fallback: in g->dense.gpatch, written by gmm_best_kernel's blocks)
    if (!lse_screened && !marginalize && !fused) {
      if ((rc = bucketed_backward(g, flux, grid, n_begin, n_end, arg, s, patch_norm))) return rc;
    }

    g->pass = GmmPass{true, H, W, stride, shift_y, shift_x, patch_row_begin, patch_row_end, marginalize, fused, lse_screened, g->screen.gen, shift_dev, norm, patch_norm};
    if (!(phases & 2)) return JD_OK;
  } else {
    const GmmPass& ps = g->pass;
    JD_REQUIRE(ps.valid && ps.H == H && ps.W == W && ps.stride == stride && ps.shift_y == shift_y && ps.shift_x == shift_x &&
                   ps.row_begin == patch_row_begin && ps.row_end == patch_row_end && ps.marginalize == marginalize &&
                   ps.gen == g->screen.gen && ps.shift_dev == shift_dev && grad_flux_accum && ps.norm.kind == norm.kind &&
                   ps.norm.p0 == norm.p0 && ps.norm.p1 == norm.p1 && ps.patch_norm == patch_norm,
               "jd_gmm_prior_fwd_bwd: phase 2 (gather) without the matching phase 1 of the same pass");
    fused = ps.fused, lse_screened = ps.lse_screened;
  }
  g->pass.valid = false;
  GmmGatherArgs ga{};
  set_patch_grid(ga, grid);
  ga.gpatch = g->dense.gpatch.ptr, ga.grad = grad_flux_accum, ga.nPy = nPy, ga.row_begin = patch_row_begin, ga.row_end = patch_row_end;
  ga.y_begin = patch_row_begin * stride;
  ga.y_end = (patch_row_end - 1) * stride + P;
  ga.coef = grad_coef;
  ga.band = band_out;
  ga.norm = norm, ga.raw_flux = raw_flux;
  if (fused) ga.winner = g->fused.winner.ptr, ga.grec = g->fused.grec.ptr, ga.flag = g->screen.ctl.ptr, ga.gen = g->screen.gen;
  ga.vec = W % 4 == 0 && aligned16(grad_flux_accum) && (!has_norm || aligned16(raw_flux)) ? 1 : 0;
  if (step) {
    ga.do_step = 1, ga.step = *step, ga.y_begin = 0, ga.y_end = H;  // every pixel of the image takes the step
    ga.preload = opt_value(OPT_GMM_GATHER_PRELOAD, 1) != 0;
    ga.vec = ga.vec && aligned16(step->theta) && aligned16(step->flux_in) && aligned16(step->flux_out) &&
             aligned16(step->grad_flux) && aligned16(step->m) && aligned16(step->v) && aligned16(step->mask);
    for (int k = 0; k < ADDEND_MAX; ++k) ga.vec = ga.vec && aligned16(step->addend[k]);
  }
  return launch_gather(ga, s);
}

// jd_gmm_prior_fwd_bwd under the image norm `norm`: 16x16 patches take the whole-image pass of gmm256.hip, or a refusal
static int gmm_prior_pass(jd_gmm* g, const ImageNormArgs& norm, const float* flux, int H, int W, int stride, int shift_y,
                          int shift_x, int patch_row_begin, int patch_row_end, int marginalize, float value_scale,
                          float* value_out, int accumulate_value, float grad_coef, float* grad_flux_accum, int32_t* argmax_out,
                          const int* shift_dev, int phases, void* stream) {
  if (g->d256) {
    JD_REQUIRE(flux && value_out, "jd_gmm_prior_fwd_bwd: null argument");
    JD_REQUIRE(phases == 3, "jd_gmm_prior_fwd_bwd: D = 256 handles run whole passes only (phases = %d, need 3)", phases);
    JD_REQUIRE(H >= 16 && W >= 16 && stride >= 1, "jd_gmm_prior_fwd_bwd: image (%d, %d) / stride %d not valid for D = 256", H, W, stride);
    const int nPy256 = (H - 16) / stride + 1;
    JD_REQUIRE(patch_row_begin == 0 && (patch_row_end < 0 || patch_row_end == nPy256),
               "jd_gmm_prior_fwd_bwd: D = 256 handles take no patch row shard ([%d, %d) of %d rows)", patch_row_begin,
               patch_row_end, nPy256);
    hipStream_t s = as_stream(stream);
    const float* image = flux;
    if (norm.kind != NORM_IDENTITY) {
      int rc;
      if ((rc = g->normed.reserve((size_t)H * W))) return rc;
      if ((rc = launch_image_norm(flux, g->normed.ptr, (size_t)H * W, norm, g->n_cu, s))) return rc;
      image = g->normed.ptr;
    }
    return gmm256_prior(g->d256, image, flux, norm, H, W, stride, shift_y, shift_x, marginalize, value_scale, value_out,
                        accumulate_value, grad_coef, grad_flux_accum, argmax_out, shift_dev, s, g->patch_norm);
  }
  return gmm_prior_impl(g, norm, flux, H, W, stride, shift_y, shift_x, patch_row_begin, patch_row_end, marginalize, value_scale,
                        value_out, accumulate_value, grad_coef, grad_flux_accum, argmax_out, nullptr, stream, nullptr, shift_dev,
                        phases);
}

int jd::gmm_prior_whole(jd_gmm* g, const ImageNormArgs& norm, const float* flux, int H, int W, int stride, int shift_y,
                        int shift_x, int marginalize, float value_scale, float* value_out, int accumulate_value,
                        float grad_coef, float* grad_flux_accum, int32_t* argmax_out, const int* shift_dev, void* stream) {
  return gmm_prior_pass(g, norm, flux, H, W, stride, shift_y, shift_x, 0, -1, marginalize, value_scale, value_out,
                        accumulate_value, grad_coef, grad_flux_accum, argmax_out, shift_dev, 3, stream);
}

extern "C" int jd_gmm_prior_fwd_bwd(jd_gmm* g, const float* flux, int H, int W, int stride, int shift_y,
                                    int shift_x, int patch_row_begin, int patch_row_end, int marginalize,
                                    float value_scale, float* value_out, int accumulate_value, float grad_coef,
                                    float* grad_flux_accum, int32_t* argmax_out, const int* shift_dev, int phases,
                                    void* stream) {
  JD_REQUIRE(g, "jd_gmm_prior_fwd_bwd: null argument");
  return gmm_prior_pass(g, g->norm, flux, H, W, stride, shift_y, shift_x, patch_row_begin, patch_row_end, marginalize,
                        value_scale, value_out, accumulate_value, grad_coef, grad_flux_accum, argmax_out, shift_dev, phases,
                        stream);
}

extern "C" int jd_gmm_prior_fwd_bwd_step(jd_gmm* g, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                                         int marginalize, float value_scale, float* value_out, int accumulate_value,
                                         float grad_coef, const jd_step* step, const int* shift_dev, int phases,
                                         void* stream) {
  JD_REQUIRE(!(g && g->d256), "jd_gmm_prior_fwd_bwd_step: D = 256 handles have no fused optimizer step");
  JD_REQUIRE(step && step->theta && step->flux_in && step->flux_out && step->grad_flux, "jd_gmm_prior_fwd_bwd_step: null argument");
  JD_REQUIRE(step->sgd || (step->exp_avg && step->exp_avg_sq), "jd_gmm_prior_fwd_bwd_step: Adam needs its moment images");
  AdamArgs a{};
  a.theta = step->theta, a.flux_in = step->flux_in, a.flux_out = step->flux_out, a.grad_flux = const_cast<float*>(step->grad_flux);
  a.m = step->exp_avg, a.v = step->exp_avg_sq, a.mask = step->mask, a.n = (size_t)H * W;
  a.step_size = step->step_size, a.beta1 = step->beta1, a.beta2 = step->beta2, a.one_minus_beta1 = step->one_minus_beta1;
  a.one_minus_beta2 = step->one_minus_beta2, a.bias2_sqrt = step->bias2_sqrt, a.eps = step->eps, a.lr = step->lr;
  a.zero_grad = 0, a.sgd = step->sgd ? 1 : 0, a.linear = step->use_log_flux ? 0 : 1, a.bias_dev = step->bias_dev;
  static_assert(ADDEND_MAX == JD_ADDEND_MAX, "jd_step::addend and AdamArgs::addend");
  for (int k = 0, live = 1; k < ADDEND_MAX; ++k) {  // (the leading non-null entries count)
    live = live && step->addend[k] != nullptr;
    a.addend[k] = live ? step->addend[k] : nullptr;
  }
  JD_REQUIRE(g, "jd_gmm_prior_fwd_bwd: null argument");
  return gmm_prior_impl(g, g->norm, flux, H, W, stride, shift_y, shift_x, 0, -1, marginalize, value_scale, value_out,
                        accumulate_value, grad_coef, nullptr, nullptr, nullptr, stream, &a, shift_dev, phases);
}

extern "C" int jd_gmm_prior_band_fwd_bwd(jd_gmm* g, const float* flux, int H, int W, int stride, int shift_y,
                                         int shift_x, int patch_row_begin, int patch_row_end, int marginalize,
                                         float value_scale, float* value_out, int accumulate_value, float grad_coef,
                                         float* band_out, void* stream) {
  JD_REQUIRE(!(g && g->d256), "jd_gmm_prior_band_fwd_bwd: D = 256 handles have no band output");
  JD_REQUIRE(band_out, "jd_gmm_prior_band_fwd_bwd: null band");
  JD_REQUIRE(g, "jd_gmm_prior_fwd_bwd: null argument");
  return gmm_prior_impl(g, g->norm, flux, H, W, stride, shift_y, shift_x, patch_row_begin, patch_row_end, marginalize,
                        value_scale, value_out, accumulate_value, grad_coef, nullptr, nullptr, band_out, stream);
}

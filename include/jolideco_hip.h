/*
 * jolideco_hip.h -- C-ABI of libjolideco_hip.so: the MI355X (gfx950) implementation of the
 * Jolideco MAP-deconvolution inner loop.
 *
 * The reference (pure Python/PyTorch, /root/reference) has no FFI for this path; its seam is the
 * Python object protocol.  Each entry point below names the reference code it replaces
 * (file:line relative to the reference root).  INTEGRATION.md shows the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, a negative jd_status otherwise; the message of the
 *     last failure on the calling thread is available from jd_last_error()
 *   - all `float*` image arguments are DEVICE pointers to contiguous row-major fp32 (H, W)
 *     images borrowed from the caller (PyTorch owns them); handles own their workspaces
 *   - all work is enqueued asynchronously on the `stream` argument (a hipStream_t passed as
 *     void*); no call synchronises except *_create and *_destroy
 *   - scalar outputs (`*_out`) are DEVICE pointers to one float
 *   - no C++ exceptions cross this boundary; handles are not thread-safe, and a handle belongs to ONE stream at a
 *     time (its work buffers and cached device tables are reused from call to call without cross-stream events)
 */
#ifndef JOLIDECO_HIP_H
#define JOLIDECO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  JD_OK = 0,
  JD_ERR_INVALID = -1, /* bad argument / unsupported shape */
  JD_ERR_HIP = -2,     /* a HIP runtime call failed */
  JD_ERR_FFT = -3,     /* a rocFFT call failed */
  JD_ERR_ALLOC = -4
} jd_status;

#define JD_MAX_COMPONENTS 8

typedef struct jd_conv_plan jd_conv_plan; /* FFT-convolution geometry + rocFFT plans + workspaces */
typedef struct jd_gmm jd_gmm;             /* GMM constants in MFMA fragment order + workspaces */

/* library ------------------------------------------------------------------------------- */
int jd_version(void);
const char* jd_last_error(void);
/* number of HIP devices visible / name of the compiled target ("gfx950") */
const char* jd_target_arch(void);

/* Tuning / test switches (new; the reference has none).  Every switch has the name of the environment variable that
 * sets its initial value when the library is loaded (JD_GMM_SCREEN, JD_SEP_WALK, JD_SEP_NO_ALIAS, ...; the full list is
 * the table in csrc/options.hip); after loading, the environment is never read again by a launch path -- a test or an
 * A/B tool that wants another variant calls jd_set_option(key, "value"), or (key, NULL) to return to the default.
 * Unknown keys are an error.  jd_get_option: *is_set / *value of the switch as the library sees it now. */
int jd_set_option(const char* key, const char* value);
int jd_get_option(const char* key, int* is_set, int* value);

/* Convolution plan --------------------------------------------------------------------------
 * Replaces the per-call shape logic of jolideco/utils/torch.py:363-370 (`convolve_fft_torch`):
 * linear "same" convolution of an (H, W) image with a (kh, kw) kernel, zero outside the image; the
 * crop offset is the reference's `_centered` offset ((kh-1)/2, (kw-1)/2) (utils/torch.py:337-344).
 * Two methods compute the same function:
 *   FFT    where the padded lengths are of the form 2^a * {1, 3, 9} (<= 9216 columns, <= 4608 rows per image half: images
 *          up to 9216 columns x 9216 rows less the PSF's halo), an image half holds the PSF and W >= 8: hand-written transforms on the un-padded grid (csrc/fftnative.hip: rows, columns with the
 *          k-space product, rows^-1 with the epilogue; the likelihood step of a dataset in five launches, with
 *          up-sampling and calibration too); otherwise rocFFT R2C / k-space multiply / C2R on a zero padded (Hp, Wp)
 *          grid, Hp >= H+kh-1, Wp >= W+kw-1 rounded up to FFT-friendly (2,3,5-smooth, Wp % 4 == 0) sizes
 *          (JD_CONV_MODE_FFT_EXACT forces rocFFT on the reference's own grid (H+kh-1, W+kw-1));
 *   DIRECT the sum over PSF taps as Toeplitz products on the matrix cores, PSFs up to 33x33; padding, exposure
 *          scaling and crop are folded into the kernel (csrc/directconv.hip).  Default where the operands fit in LDS
 *          (up to ~25x33): both operands split into two fp16 terms (22 significant bits, three fp16 MFMAs per
 *          product, fp32 accumulation; relative error of a convolution ~1e-6 of its maximum); otherwise, or with
 *          option JD_DIRECT_FP32=1, the fp32-input MFMA kernel (an exact fmaf chain).
 *   SEPARABLE for a PSF that is a sum of at most 3 outer products u_r v_r^T (a sampled Gaussian is 1, a
 *          double Gaussian 2): a row pass and a column pass of kh + kw taps per rank instead of kh * kw,
 *          PSFs up to 68x68 (csrc/sepconv.hip).  Whether a PSF qualifies is decided by
 *          jd_psf_separable_rank() / jd_conv_psf_spectrum(); a PSF that does not is an error for such a plan.
 * JD_CONV_MODE_AUTO picks DIRECT when the PSF is small enough for it to be faster than FFT -- up to 17 taps; up to 33
 * where the native FFT sizes do not fit, on images below 2^20 pixels, or with option JD_DIRECT_AUTO_ALL (so a general PSF
 * of 18 to 33 taps on an image of 4600 to 9216 columns or rows takes the native FFT plan, no longer DIRECT) --; it never picks
 * SEPARABLE, because the choice depends on the PSF values, which a plan does not know: the caller asks
 * jd_psf_separable_rank() and requests JD_CONV_MODE_SEPARABLE (jolideco_amd.NPredModel does). */
enum {
  JD_CONV_MODE_AUTO = 0,
  JD_CONV_MODE_FFT_EXACT = 1,
  JD_CONV_MODE_FFT = 2,
  JD_CONV_MODE_DIRECT = 3,
  JD_CONV_MODE_SEPARABLE = 4
};
/* Rank R (1..3) of the outer-product decomposition of a (kh, kw) PSF given in HOST memory, or 0 when the PSF
 * is not that low-rank to within `tol` (sum |psf - sum_r u_r v_r^T| <= tol * sum |psf|; tol <= 0 selects the
 * default 3e-7, a few fp32 ulps) or larger than 68x68.  Host-only analysis, no device work. */
int jd_psf_separable_rank(const float* psf_host, int kh, int kw, float tol);
int jd_conv_plan_create(int H, int W, int kh, int kw, int mode, jd_conv_plan** plan_out);
int jd_conv_plan_destroy(jd_conv_plan* plan);
/* shape[0..5] = {H, W, Hp, Wp, oy, ox}; (Hp, Wp) = (H, W) for the direct method */
int jd_conv_plan_shape(const jd_conv_plan* plan, int* shape6);
/* 0 = FFT, 1 = DIRECT, 2 = SEPARABLE */
int jd_conv_plan_method(const jd_conv_plan* plan);
/* 1 when a plan of this geometry with the FFT method runs the hand-written transforms of csrc/fftnative.hip (and with them
 * the batched joint steps), 0 when it runs rocFFT (a size the native kernels do not cover -- padded rows beyond 9216 points,
 * padded image halves beyond 4608 rows, images narrower than 8 pixels or shorter than two PSFs -- or option JD_FFT_NATIVE=0).
 * A native plan of the largest size holds 0.64 GB of work arrays and 0.34 GB per kernel spectrum; jd_conv_plan_create
 * answers JD_ERR_ALLOC where the device has no room for them.
 * Host logic only, no device needed: a caller that is about to embed PSFs of different sizes in one array so that their
 * datasets share a plan (jolideco_amd/models/npred.py common_kernel_shape) asks first. */
int jd_conv_native_fft_supported(int H, int W, int kh, int kw);
/* 1 when a SEPARABLE plan runs a launch over `n_datasets` datasets (1 = the per-dataset calls) on the strip-walk kernels
 * of csrc/walkconv.hip instead of the tile kernel of csrc/sepconv.hip, given rank-1 operators (PSFs up to 17 x 17, image
 * width a multiple of 4, enough pixels x datasets to fill the chip; option JD_SEP_WALK = 0 / 1 forces either).  Both
 * compute the same function; a benchmark uses this to name the kernel it timed. */
int jd_conv_plan_takes_walk(const jd_conv_plan* plan, int n_datasets);
/* Which kernels a likelihood step of `n_datasets` datasets (1 = the per-dataset call) with up-sampling factor `upsampling`
 * launches on this plan -- asked of the functions the launch path itself asks; read-only, no device work.  A test uses it
 * to pin a case to the kernel it means to check.  route8 =
 *   [0], [1]  Nx, Ny: lengths of the native row / column transforms (0: not a native FFT plan)
 *   [2], [3]  row schedule of the forward-row launch and of the pooled middle launch: 0 generic-large, 1 2304, 2 4608,
 *             3 1152, 4 generic-small, 5 one-wave tiny, 6 generic-huge (rows beyond 4608 points or 5120 pixels, up to
 *             9216: 768 threads per row pair); -1: no such launch
 *   [4]       1 when the fused up-sampled (pooled) launches take this factor and grid
 *   [5]       1 when the column passes exchange pooled row groups with the middle launch
 *   [6]       jd_npred_poisson_calibrated_batch_fwd_bwd: 0 per-dataset calls, 1 every launch over all datasets,
 *             2 the FFT launches dataset by dataset and the tail over all
 *   [7]       transposed shift: R = 1, 2, 4 rows per thread of the four-pixel kernel (16-byte aligned images), 0 scalar kernels */
int jd_conv_plan_step_route(const jd_conv_plan* plan, int upsampling, int n_datasets, int32_t* route8);
/* Which kernels a plain convolution, its adjoint and the un-up-sampled likelihood step launch on a plan of the native FFT
 * path -- asked of the function the column launch itself asks for its table entry, and of the row launches' schedule
 * function; read-only, no device work; JD_ERR_INVALID for any other plan.  route8 =
 *   [0], [1]  Nx, Ny: lengths of the row / column transforms
 *   [2]       lanes (threads) per column: 64, 128 or 256
 *   [3]       columns per block actually launched (option JD_FFT_NATIVE = 2 / 4 / 8 forces it where the table entry that
 *             leads to can be launched with lanes x columns threads; otherwise the default stands)
 *   [4]       1: a compile-time entry of the column table, 0: the generic kernel of that many lanes
 *   [5]       row schedule (numbered as in jd_conv_plan_step_route) of a forward-row launch over `n_datasets` datasets
 *   [6]       row schedule of the single-image inverse-row launch
 *   [7]       0 (reserved) */
int jd_conv_plan_fft_route(const jd_conv_plan* plan, int n_datasets, int32_t* route8);
/* Which instantiation of the MFMA Toeplitz kernel (csrc/directconv.hip) a DIRECT plan launches -- computed by the functions
 * the launch itself calls, from the plan's own fields; read-only, no device work; an error for a plan of another method.
 * kernel4 =
 *   [0]  KC, the input columns of one Toeplitz product: fp32 kernel 16, 20, .. 48 (15 + kw rounded up to a multiple of 4),
 *        split-fp16 kernel 32 (kw <= 17) or 64
 *   [1]  1: the split-fp16 kernel, 0: the fp32 one (a PSF whose planes and table do not fit in LDS, or JD_DIRECT_FP32=1)
 *   [2]  1 when the forward convolution stages its window in 16-byte chunks, given 16-byte aligned images (the shape part
 *        of the condition: W % 4 == 0 and the window's first column a multiple of 4); 0: element by element
 *   [3]  the same for the adjoint
 * (The float4 epilogue has a condition of its own: W % 4 == 0 and every image it touches 16-byte aligned.) */
int jd_conv_plan_direct_kernel(const jd_conv_plan* plan, int32_t* kernel4);
/* The frame -- 17 or 33 taps per direction -- in which the strip-walk kernels run the operator `khat` that
 * jd_conv_psf_spectrum built for this SEPARABLE plan, or 0 when they do not take it (rank > 1, non-zero taps wider than 33,
 * a buffer the library did not build).  The frame follows from the NON-ZERO taps of the operator, not from the plan's
 * (kh, kw): a 17 x 17 PSF embedded in a 33 x 33 array of zeros (datasets with different PSF sizes share one plan -- and one
 * batched joint step -- that way) walks in the 17-tap frame. */
int jd_conv_operator_walk_frame(const jd_conv_plan* plan, const float* khat);
/* The library remembers, by device address, what it knows about every SEPARABLE operator buffer it built (rank, support of
 * the taps).  A caller that frees such a buffer tells the library so: a later allocation at the same address is then an
 * unknown buffer again (and takes the general kernels) until jd_conv_psf_spectrum fills it. */
int jd_conv_operator_forget(const float* khat);
/* HALF the number of floats of one per-(dataset, component) kernel operator buffer `khat`:
 * FFT: complex64 elements of the kernel spectrum, Hp * (Wp/2 + 1); DIRECT: floats of one Toeplitz
 * fragment table (the buffer holds the forward and the adjoint table); SEPARABLE: the rank and the row /
 * column taps of both directions (a few hundred floats). */
size_t jd_conv_plan_spectrum_size(const jd_conv_plan* plan);

/* Kernel operator of one PSF, computed ONCE per (dataset, component) and cached by the caller in
 * `khat` (device, 2*spectrum_size floats).  FFT: K-hat = rfft2(psf, s=(Hp, Wp)) / (Hp*Wp); DIRECT: the
 * PSF in MFMA fragment order (forward and flipped).  Replaces the per-call
 * `torch.fft.rfft2(kernel, s=shape)` of utils/torch.py:368 (and the unused cache of
 * models/npred.py:117-127).  The 1/(Hp*Wp) of the unnormalised inverse transform is folded in. */
int jd_conv_psf_spectrum(jd_conv_plan* plan, const float* psf, float* khat, void* stream);

/* out[H,W] = crop( irfft2( rfft2(pad(image * scale_image)) * khat ) ); scale_image may be NULL.
 * Stand-alone `convolve_fft_torch` (utils/torch.py:347-370); used at setup for the exposure edge
 * correction of models/npred.py:108-113 and by NPredModel.forward (npred.py:175-179). */
int jd_conv_same(jd_conv_plan* plan, const float* image, const float* scale_image, const float* khat,
                 float* out, void* stream);

/* Fused forward model + Poisson NLL + gradient for ONE dataset and n_comp flux components.
 * Replaces, per optimizer step (jolideco/core.py:217-221,228):
 *   NPredModels.evaluate            models/npred.py:210-261  (sum_c clip(conv(flux_c*E_c, psf_c),0) + bkg)
 *   NPredModel.forward              models/npred.py:160-191  (upsampling_factor 1, no rmf)
 *   convolve_fft_torch              utils/torch.py:347-370
 *   nn.PoissonNLLLoss(log_input=False, reduction="mean", eps, full=True)   loss.py:35-37
 *   and the autograd backward of all of the above down to d loss / d flux_c.
 * loss_out      <- mean(n - c*log(n+eps)) + stirling_mean        (device scalar)
 * grad_flux[c]  <- (accumulate ? += : =) grad_scale * E_c * corr(psf_c, g * [conv_c >= 0]),
 *                  g = (1 - c/(n+eps)) / (H*W);  pass grad_flux == NULL for a forward-only
 *                  evaluation (PoissonLoss.evaluate, loss.py:56-71).
 * npred_out     optional output of the total predicted counts (counts grid).
 * upsampling    u >= 1: flux_c, exposure_c and grad_flux_c live on the plan's (H, W) grid, background,
 *               counts and npred_out on (H/u, W/u); the convolution is sum-pooled u x u before the clip
 *               (models/npred.py:181-184, `upsampling_factor`).  The PSF given to jd_conv_psf_spectrum and
 *               the exposure must already be up-sampled (models/npred.py:96-106 does that at setup).
 * `stirling_mean` = mean([c>1] * (c*log c - c + 0.5*log(2*pi*c))) is flux independent and is
 * supplied by the caller (computed once per dataset). */
int jd_npred_poisson_fwd_bwd(jd_conv_plan* plan, int n_comp, const float* const* flux,
                             const float* const* exposure, const float* const* khat,
                             const float* background, const float* counts, float stirling_mean,
                             float eps, float* loss_out, float* const* grad_flux, int accumulate,
                             float grad_scale, float* npred_out, int upsampling, void* stream);

/* The same step for ONE dataset whose n_comp flux components live on grids of DIFFERENT up-sampling factors
 * (`upsampling_factor` is an attribute of each SpatialFluxComponent, and NPredModels.from_dataset_numpy builds one
 * NPredModel per component with that component's factor, models/npred.py:279-295): component c has its own plan on the
 * (Hc * u_c, Wc * u_c) grid, (Hc, Wc) the counts grid, and its own factor u_c >= 1.
 *   pooled_c      = sumpool_{u_c}( PSF_c (*) (flux_c x E_c) )                        models/npred.py:160-191
 *   n             = sum_c max(pooled_c, 0) + background                              models/npred.py:241-261
 *   loss_out     <- mean(n - c*log(n+eps)) + stirling_mean                           loss.py:35-37
 *   grad_flux[c] <- (accumulate ? += : =) grad_scale * E_c * corr(PSF_c, replicate_{u_c}( g * [pooled_c >= 0] )),
 *                   g = (1 - c/(n+eps)) / (Hc*Wc)
 * Every component's convolution and adjoint run on that component's plan by the plan's own method (separable, direct,
 * native FFT, rocFFT); between them ONE launch over the counts grid reads component c's convolution with plan c's row
 * pitch, crop offset and factor, sum-pools, clips per component, adds the background, accumulates the loss, writes
 * npred_out and writes the masked, u_c x u_c-replicated g straight into plan c's adjoint input.
 *   plans, flux, exposure, khat, grad_flux, upsampling : host arrays of n_comp entries (grad_flux nullable: forward
 *                   only); flux[c], exposure[c], grad_flux[c] on plan c's grid; plans may repeat
 *   background, counts, npred_out (nullable)           : on the counts grid
 * Every plan's image shape must be exactly upsampling[c] times one common counts shape, and every factor lies in
 * [1, 8] as in jd_npred_poisson_fwd_bwd (JD_ERR_INVALID otherwise).
 * The work buffers belong to the plans: after the first call with a set of plans the call neither allocates nor
 * synchronises.  All other arguments as in jd_npred_poisson_fwd_bwd. */
int jd_npred_poisson_mixed_fwd_bwd(jd_conv_plan* const* plans, int n_comp, const float* const* flux,
                                   const float* const* exposure, const float* const* khat, const float* background,
                                   const float* counts, float stirling_mean, float eps, float* loss_out,
                                   float* const* grad_flux, int accumulate, float grad_scale, float* npred_out,
                                   const int* upsampling, void* stream);

/* The joint step over SEVERAL datasets in three launches instead of four per dataset (new: the reference has no joint
 * mode; this is the batched form of the loop `for dataset: jd_npred_poisson_fwd_bwd(..., accumulate = dataset > 0)` that
 * jolideco_amd's fit_mode="joint" runs, jolideco/core.py:214-229 being its per-dataset counterpart).  Restrictions: one
 * flux component, no up-sampling, no calibration, ONE plan shared by all datasets (same image and PSF array shape) with
 * the SEPARABLE method or with the FFT method on the native transforms (then every launch of the likelihood step covers
 * all datasets: csrc/fftnative.hip; a forward-only call and option JD_FFT_BATCH=0 run the per-dataset calls); at most 16
 * datasets per call.  Same results as the loop, bit for bit (the per-dataset gradient contributions are added in
 * dataset order).
 *   exposure, khat, background, counts, loss_out : host arrays of n_datasets device pointers
 *   stirling_mean                                : host array of n_datasets floats
 *   grad_flux                                    : nullable (forward only) */
int jd_npred_poisson_batch_fwd_bwd(jd_conv_plan* plan, int n_datasets, const float* flux, const float* const* exposure,
                                   const float* const* khat, const float* const* background,
                                   const float* const* counts, const float* stirling_mean, float eps,
                                   float* const* loss_out, float* grad_flux, int accumulate, float grad_scale,
                                   void* stream);

/* jd_npred_poisson_batch_fwd_bwd (accumulate = 0, grad_flux required) that may leave part of the gradient in images of its
 * own.  Where the datasets' PSFs walk in both strip-walk frames (17 and 33 taps), all datasets of one frame come in front
 * of all of the other and the second frame has m <= JD_ADDEND_MAX datasets, the adjoints of those m datasets are not added
 * into grad_flux: dataset (n_datasets - m + i) writes grad_scale * exposure * corr(g, psf) -- the very number the call
 * above adds -- to addends[i], in a launch of its own that runs beside the first frame's adjoint launch on stream2.
 * *n_addends <- m, and the gradient of the step is
 *     ((grad_flux + addends[0]) + addends[1]) + ...        in this order: the bits of jd_npred_poisson_batch_fwd_bwd,
 * which jd_adam_step_addends and jd_gmm_prior_fwd_bwd_step (jd_step.addend) form while they read the gradient.
 * Everywhere else (one frame, frames interleaved, more late datasets than images, other kernels, option
 * JD_SEP_ADJ_ADDENDS = 0) the call IS jd_npred_poisson_batch_fwd_bwd and *n_addends <- 0.
 *   addends : host array of JD_ADDEND_MAX device images (H x W floats, 16-byte aligned), the leading non-null ones usable
 *   stream2 : nullable (then everything runs on stream).  The call forks stream2 behind the forward launch on stream and
 *             joins it into stream before it returns: work enqueued on stream afterwards sees the addends complete, and a
 *             stream capture sees a closed parallel branch.  stream2 must not be the stream of other work of the step. */
#define JD_ADDEND_MAX 4
int jd_npred_poisson_batch_addends_fwd_bwd(jd_conv_plan* plan, int n_datasets, const float* flux,
                                           const float* const* exposure, const float* const* khat,
                                           const float* const* background, const float* const* counts,
                                           const float* stirling_mean, float eps, float* const* loss_out, float* grad_flux,
                                           int accumulate, float grad_scale, float* const* addends, void* stream2,
                                           int* n_addends, void* stream);

/* The batched joint step for SEVERAL flux components (NPredModels.evaluate sums the per-component models after their
 * clip, models/npred.py:210-261; per-component PSF / exposure as in npred.py:281-295): dataset d convolves flux[c] with
 * khat[d * n_components + c] after scaling by exposure[d * n_components + c]; one forward launch (grid.y = dataset, the
 * components walked inside the block), one loss launch and one adjoint launch per component.  Restrictions as above;
 * at most 4 components.  Same results as the per-dataset loop, bit for bit.
 *   flux, grad_flux     : host arrays of n_components device pointers (grad_flux nullable: forward only)
 *   exposure, khat      : host arrays of n_datasets * n_components device pointers, dataset major */
int jd_npred_poisson_batch_multi_fwd_bwd(jd_conv_plan* plan, int n_datasets, int n_components, const float* const* flux,
                                         const float* const* exposure, const float* const* khat,
                                         const float* const* background, const float* const* counts,
                                         const float* stirling_mean, float eps, float* const* loss_out,
                                         float* const* grad_flux, int accumulate, float grad_scale, void* stream);

/* The same with the per-dataset calibration of NPredCalibration (models/npred.py:298-402,225-237):
 *   shift_xy             device [2] = {shift_x, shift_y} in COUNTS pixels or NULL: every flux_c is shifted
 *                        (bilinear, zero padding = shift_image_torch, utils/torch.py:196-223) before the
 *                        exposure / PSF are applied; scale = upsampling
 *   log_background_norm  device [1] or NULL: background * exp(.)
 *   grad_shift_xy        device [2] or NULL  <- grad_scale * d loss / d shift_xy   (summed over components)
 *   grad_log_background_norm  device [1] or NULL  <- grad_scale * d loss / d log_background_norm
 * The parameters are read from device memory so that a fit never synchronises on them.  The caller
 * decides whether the shift is active (the reference skips it -- and its gradient -- while it is ~0). */
int jd_npred_poisson_calibrated_fwd_bwd(jd_conv_plan* plan, int n_comp, const float* const* flux,
                                        const float* const* exposure, const float* const* khat,
                                        const float* background, const float* counts, float stirling_mean,
                                        float eps, float* loss_out, float* const* grad_flux, int accumulate,
                                        float grad_scale, float* npred_out, int upsampling, const float* shift_xy,
                                        const float* log_background_norm, float* grad_shift_xy,
                                        float* grad_log_background_norm, void* stream);

/* The joint step over SEVERAL datasets of ONE flux component with the per-dataset calibration and / or up-sampling (the
 * fits of the reference's examples: examples/chandra-e0102-filament.py:178-203): the batched form of the loop
 * `for dataset: jd_npred_poisson_calibrated_fwd_bwd(..., accumulate = dataset > 0)` -- same results, bit for bit.  On a
 * plan of the native FFT convolution with up-sampling 2 or 4 every launch covers all datasets: rows (with the dataset's
 * shift), columns, the pooled Poisson launch, the adjoint's column pass, rows^-1 + adjoint epilogue into one image per
 * dataset, a transposed shift that adds the datasets up in dataset order, and the finalize of the shift gradients (at
 * every size since round 5; option JD_FFT_BATCH=0 runs the per-dataset calls, 3 / 4 the intermediate forms measured in
 * csrc/fftconv.hip).  Every other case runs the per-dataset calls.
 *   exposure, khat, background, counts, loss_out : host arrays of n_datasets device pointers
 *   shift_xy, log_background_norm, grad_shift_xy, grad_log_background_norm : NULL, or host arrays of n_datasets device
 *                                                  pointers with NULL entries where a dataset has none (see above) */
int jd_npred_poisson_calibrated_batch_fwd_bwd(jd_conv_plan* plan, int n_datasets, const float* flux,
                                              const float* const* exposure, const float* const* khat,
                                              const float* const* background, const float* const* counts,
                                              const float* stirling_mean, float eps, float* const* loss_out,
                                              float* grad_flux, int accumulate, float grad_scale, int upsampling,
                                              const float* const* shift_xy, const float* const* log_background_norm,
                                              float* const* grad_shift_xy, float* const* grad_log_background_norm,
                                              void* stream);

/* Same chain split at the reference's object seams, for callers that keep the reference's own
 * loop structure (autograd.Function wrappers in jolideco_amd/ops.py):
 * conv_padded[c] are plan-owned buffers exposed through jd_conv_plan_conv_buffer. */
int jd_poisson_nll(const float* npred, const float* counts, size_t n, float stirling_mean, float eps,
                   float* loss_out, float* grad_npred /* nullable; (1 - c/(n+eps))/n_total */,
                   void* stream);
/* grad_image (+)= scale_image * crop_adjoint( irfft2( rfft2(pad(grad_out)) * conj(khat) ) ):
 * the adjoint of jd_conv_same (autograd of utils/torch.py:367-370). */
int jd_conv_same_adjoint(jd_conv_plan* plan, const float* grad_out, const float* scale_image,
                         const float* khat, float* grad_image, int accumulate, void* stream);

/* GMM patch prior ------------------------------------------------------------------------
 * jd_gmm_create takes HOST pointers to the fp32 constants of
 * jolideco/priors/patches/gmm.py: precisions_cholesky (K, D, D) (:139-149, utils/numpy.py:16-34),
 * means_precisions_cholesky (K, D) (:217-228), const_k[k] = -0.5*D*log(2*pi) + log_det_cholesky[k]
 * + log_weights[k] (:235-240,114-117,276-281) and pixel_weights (D,) (:283-299).  D must be 64
 * (8x8 patches) or 256 (16x16 patches), K <= 4096; any other D returns JD_ERR_INVALID.  The library re-lays them out in
 * MFMA fragment order with sqrt(pixel_weight) folded into the columns.
 * D = 256 HANDLES (csrc/gmm256.hip) have ONE path, dense fp32 on v_mfma_f32_16x16x4_f32 -- no fp16 screen, every component
 * is evaluated for every patch, the logsumexp is the exact one over all K -- and a narrower interface:
 *   jd_gmm_prior_fwd_bwd       the whole image only (patch_row_begin = 0, patch_row_end = -1 or the number of patch rows)
 *                              and the whole pass only (phases = 3); argmax_out, shift_dev, marginalize, accumulate_value and
 *                              the handle's image norm as for D = 64; patch size 16, stride in [1, 16], H, W >= 16;
 *   jd_gmm_estimate_log_prob   x: (n, 256);
 *   jd_gmm_set_image_norm, jd_gmm_set_patch_norm, jd_gmm_is_triangular, jd_gmm_screen_stats (no screened pass: generation 0),
 *   jd_gmm_destroy as for D = 64;
 *   a patch row shard, phases 1 / 2, jd_gmm_prior_fwd_bwd_step, jd_gmm_prior_band_fwd_bwd and jd_gmm_screen_clock return
 *   JD_ERR_INVALID with a message that names D = 256 and the refused option; nothing is launched and the handle stays
 *   usable.  No D = 256 call ever reaches a D = 64 kernel.
 * The fragments of a D = 256 mixture take 2 x K x 256 KB of device memory (K = 200: 105 MB). */
int jd_gmm_create(int K, int D, const float* prec_chol, const float* mu_prec, const float* const_k,
                  const float* pixel_w, jd_gmm** gmm_out);
int jd_gmm_destroy(jd_gmm* gmm);
/* 1 when every precisions_cholesky[k] is upper triangular (what compute_precision_cholesky,
 * utils/numpy.py:16-34, produces): the kernels then skip the all-zero 16x16 blocks (40 instead of 64
 * MFMAs per component and 16 patches, bit-identical results); 0 = dense variant. */
int jd_gmm_is_triangular(const jd_gmm* gmm);

/* IMAGE NORM of the prior (jolideco/utils/norms.py:225-426; priors/patches/core.py:190 `normed = self.norm(flux)`): the
 * three jd_gmm_prior_* calls below evaluate the mixture on n(flux) and return the gradient with respect to the RAW flux.
 *   kind 0 identity   n = f                              (p0, p1 unused; the state of a new handle)
 *        1 asinh      n = asinh(f / p0) / asinh(p1 / p0)             (p0 = alpha, p1 = beta)
 *        2 fixed-max  n = clip(f / p0, 0, 1)                         (p0 = max_value)
 *        3 sigmoid    n = 1 / (1 + exp(-(f - p1 / 2) / p0))          (p0 = alpha, p1 = beta)
 *        4 atan       n = 2 atan(f / p0) / pi                        (p0 = alpha)
 *        5 log        n = log(f / p0)                                (p0 = alpha)
 *        6 power      n = (f / p1)^p0                                (p0 = alpha, p1 = beta)
 * Phase 1 of a pass with kind != 0 first writes n(flux) into an (H, W) image of the handle (one streaming kernel) and
 * every later kernel of the phase reads that image -- the `> -1e5` patch filter acts on normed values, as in the
 * reference; phase 2 multiplies every pixel's overlap-add by n'(raw flux of the pixel), (grad_coef * sum) * n', in all
 * three output forms (accumulate, band, optimizer step); a pixel whose sum is exactly 0 receives nothing (never 0 * inf).
 * The norm is a state of the HANDLE, taken by the next jd_gmm_prior_* call: callers that share a handle between priors
 * set it in front of every call.  A phase-2 call must find the norm of its phase 1 (JD_ERR_INVALID otherwise).
 * The parameters are constants (the reference trains them unless frozen). */
typedef struct {
  int kind;
  float p0, p1;
} jd_image_norm;
int jd_gmm_set_image_norm(jd_gmm* gmm, const jd_image_norm* norm);

/* PATCH NORM of the prior (jolideco/utils/norms.py:97-112; priors/patches/core.py:218 `patches = self.patch_norm(...)`):
 * what the three jd_gmm_prior_* calls below make of a patch p of the (normed, rolled) image that passed the `> -1e5` filter
 * before the mixture sees it, m = mean(p) over its D pixels:
 *   kind 0 subtract-mean       x = p - m                  (the state of a new handle)
 *        1 std-subtract-mean   x = (p - m) / m            (a float32 subtraction, then a correctly rounded division)
 * Everything behind x is the same; the gradient rows carry the norm's adjoint, kind 1:
 * dv/dp_j = (gamma_j - mean(gamma) - (gamma . x) / D) / m with gamma = dv/dx.  m = 0 gives inf / NaN as in the
 * reference (no guard).  Kind 1 always takes the dense fp32 kernels: the fp16 screen, the screened logsumexp and the
 * fused exact stage are never used for it, whatever JD_GMM_SCREEN / JD_GMM_LSE_SCREEN say (their error bounds are those
 * of mean-free patches), and jd_gmm_screen_stats' generation does not advance.  Phases, the patch row shard, the band
 * output and jd_gmm_prior_fwd_bwd_step work as for kind 0 (D = 64); D = 256 handles accept both kinds.
 * jd_gmm_estimate_log_prob takes finished patches and applies no norm.
 * Like the image norm it is a state of the HANDLE, taken by the next jd_gmm_prior_* call: callers that share a handle
 * between priors set it in front of every call.  A phase-2 call must find the patch norm of its phase 1 (JD_ERR_INVALID
 * otherwise).  Any other kind returns JD_ERR_INVALID and leaves the handle as it was. */
int jd_gmm_set_patch_norm(jd_gmm* gmm, int kind);
/* RESIDUAL OF THE CONSTANTS.  const_k of jd_gmm_create is a float32 number per component, and the caller sums its three
 * terms in float32 as the reference does: an error of up to a few 1e-5 that every patch choosing the component shares.
 * Under the subtract-mean norm a patch's value is of the order of -1e4 and that is 1e-9 of it.  Standardized patches are
 * of order 0.1: the value is c_k - q_k / 2 with both terms several times its size, and the same error is a few 1e-6 of
 * the prior value.  residual: HOST pointer to K floats, residual[k] = (c_k evaluated in float64) - (double)const_k[k].
 * The passes of patch norm kind 1 form l_k = fmaf(-0.5, q_k, const_k[k]) + residual[k] (value, arg-max and
 * responsibilities alike); the passes of kind 0, the screen and jd_gmm_estimate_log_prob never read it, so setting it
 * changes no bit of theirs.  A new handle holds zeros.  A property of the mixture, not of a pass: set it once after
 * jd_gmm_create (the call synchronises the device).  D = 256 handles accept it.  Non-finite entries: JD_ERR_INVALID. */
int jd_gmm_set_const_residual(jd_gmm* gmm, const float* residual);

/* log-prior value and gradient of GMMPatchPrior.__call__ (priors/patches/core.py:189-246) with
 * IdentityImageNorm, SubtractMeanPatchNorm (utils/norms.py:97-103), cycle-spin roll by
 * (shift_y, shift_x) (utils/torch.py:108-119), patch size 8, stride `stride`
 * (utils/torch.py:226-275), GaussianMixtureModel.estimate_log_prob (patches/gmm.py:262-281),
 * max over components (marginalize = 0) or logsumexp (marginalize = 1).  With a gradient and upper triangular
 * factors both modes go through the fp16 screen: the arg-max result is that of the dense fp32 kernel bit for bit; the
 * logsumexp leaves out terms below exp(-25) of the largest one (< 2e-9 of the sum) and is held to the reference's
 * values at 5e-5 like the dense logsumexp kernel (options JD_GMM_SCREEN=0 / JD_GMM_LSE_SCREEN=0: dense kernels).
 * Reproducibility: the arg-max mode is bit-reproducible from run to run.  The logsumexp mode with a gradient is
 * reproducible with JD_GMM_LSE_SCREEN=0 (always the dense kernels) or =2 (always the screen); by DEFAULT the library
 * decides per pass, from host-mapped statistics of earlier passes that it reads without synchronising, whether the
 * screen is worth running -- on images where it keeps overflowing, WHICH pass first skips it depends on host / GPU
 * timing, and the two paths differ at the rounding level (both within 5e-5 of the reference).
 *   value_out       <- (accumulate_value ? += : =) value_scale * sum_{patches in shard} v_patch
 *   grad_flux_accum += grad_coef * d(sum_{patches in shard} v_patch)/d flux   (NULL: forward only)
 *   argmax_out      optional int32 per patch (global patch index order), max mode only
 * Only patch rows [patch_row_begin, patch_row_end) are evaluated (multi-GPU shard of the prior;
 * pass 0 and -1 for all rows).
 * DEVICE-RESIDENT STEP SCALARS (new: what lets a whole epoch be captured in a hipGraph and replayed): with
 * shift_dev != NULL the kernels read the roll from device memory -- shift_dev[0] = shift_y in [0, H), shift_dev[1] =
 * shift_x in [0, W), the residues the host would have passed -- and ignore the two by-value arguments; every launch
 * argument of the pass is then the same from step to step (the caller uploads the shifts of the coming steps with one
 * small copy, jolideco_amd/core.py StepScalars).  Same results as the by-value form, bit for bit.
 * TWO PHASES (new: the prior beside the likelihood): `phases` = 3 runs the whole pass; 1 runs everything up to the
 * per-patch gradient rows -- value, arg-max, rows: it reads the flux and writes value_out and the handle's work buffers
 * only --, 2 the gather of those rows into grad_flux_accum (for _step: + the optimizer step).  A caller enqueues phase 1
 * on a second stream next to the likelihood launches of the step, joins the streams and calls phase 2 with the same
 * arguments (JD_ERR_INVALID if they differ or another pass of the handle ran in between); a handle has one pass in
 * flight at a time. */
int jd_gmm_prior_fwd_bwd(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y,
                         int shift_x, int patch_row_begin, int patch_row_end, int marginalize,
                         float value_scale, float* value_out, int accumulate_value, float grad_coef,
                         float* grad_flux_accum, int32_t* argmax_out, const int* shift_dev, int phases, void* stream);

/* The same evaluation with the OPTIMIZER STEP of the component in the epilogue of its last kernel (new: one pass over
 * the gradient image and one launch less per step; jolideco/core.py:229 is the step it folds in).  Where
 * jd_gmm_prior_fwd_bwd adds grad_coef * d(sum v_patch)/d flux into the gradient image, this call forms
 *   g = step->grad_flux[pixel] + grad_coef * d(sum v_patch)/d flux[pixel]      (grad_flux: all other terms, read only)
 * and applies jd_adam_step's (or jd_sgd_step's) update to every pixel of the image: theta, exp_avg, exp_avg_sq in
 * place, flux_out = exp(theta_new) [* mask].  Same bits as the two separate calls.  Whole prior only (no shard);
 * stride >= 4; JD_ERR_INVALID otherwise (the caller then makes the two calls). */
typedef struct {
  float* theta;
  const float* flux_in;
  float* flux_out;
  const float* grad_flux; /* d loss / d flux of everything but this prior */
  float* exp_avg;         /* NULL with sgd */
  float* exp_avg_sq;
  const float* mask;      /* nullable */
  float step_size, beta1, beta2, one_minus_beta1, one_minus_beta2, bias2_sqrt, eps; /* as jd_adam_step */
  float lr;               /* sgd */
  int use_log_flux, sgd;
  const float* bias_dev;  /* nullable, device [2] = {step_size, bias2_sqrt}: read by the kernel instead of the two members
                             above (the step count of a captured graph's optimizer step lives in device memory) */
  const float* addend[JD_ADDEND_MAX]; /* the leading non-null entries: images added to grad_flux in this order before the
                             prior's term, g = (grad_flux + addend[0]) + addend[1] ... (what
                             jd_npred_poisson_batch_addends_fwd_bwd left out of grad_flux); all null: none */
} jd_step;
int jd_gmm_prior_fwd_bwd_step(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                              int marginalize, float value_scale, float* value_out, int accumulate_value,
                              float grad_coef, const jd_step* step, const int* shift_dev, int phases, void* stream);

/* The same prior with `cycle_spin_subpix=True` (priors/patches/core.py:189-246; utils/torch.py:31-38,91-143): the patches
 * are cut from s = conv2d(roll(n(flux), (shift_y, shift_x)), k, padding="same"), the 3 x 3 cross-correlation of the rolled,
 * normed image with k[i][j] = wy(i - 1) * wx(j - 1), w(t) = 1 - |t - o| where |t - o| < 1, else 0 (o = x0 for columns, y0
 * for rows, both in [-0.5, 0.5]; the weights are formed in float32 as the reference's `grid_weights` does), ZERO outside
 * the rolled image.  Two streaming kernels around the unchanged pass: with (Y, X) = ((y + shift_y) mod H, (x + shift_x)
 * mod W) the rolled position of pixel (y, x), the first writes the staged image in the un-rolled frame,
 *   S[y, x] = sum_{a,b in {-1,0,1}} k[a+1][b+1] n[(y+a) mod H, (x+b) mod W] [0 <= Y+a < H] [0 <= X+b < W]
 * (the stencil wraps around the image except across the seam the roll puts at row H - shift_y and column W - shift_x, where
 * the tap is dropped); jd_gmm_prior_fwd_bwd then runs on S with the identity norm, the handle's patch norm and the same
 * roll, its gradient G = grad_coef * d(sum v_patch)/dS going to a zeroed image of the handle; the second adds
 *   dflux[y, x] = n'(flux[y, x]) sum_{a,b} k[a+1][b+1] G[(y-a) mod H, (x-b) mod W] [0 <= Y-a < H] [0 <= X-b < W]
 * to grad_flux_accum (a pixel whose sum is exactly 0 receives nothing, as in the gather).  No atomics, the nine additions
 * in row-major (a, b) order: run-to-run identical.  grad_flux_accum == NULL: value (and arg-max) only.  Value, arg-max,
 * marginalize, the image norm and the patch norm of the handle (left as found) mean what they mean for
 * jd_gmm_prior_fwd_bwd; with x0 = y0 = 0 the result is that call's, bit for bit.  The WHOLE prior only (no patch row shard,
 * no band, no phases, no fused optimizer step); D = 64 and D = 256 handles.
 * shift_dev (nullable): device [2] = roll residues in [0, H) x [0, W), read instead of shift_y / shift_x; offset_dev
 * (nullable): device [2] = {x0, y0}, read instead of x0 / y0 (captured epochs).  By-value offsets that are not finite or
 * outside [-0.5, 0.5], a NULL flux or value_out, an image smaller than a patch: JD_ERR_INVALID, nothing is launched. */
int jd_gmm_prior_subpix_fwd_bwd(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                                float x0, float y0, int marginalize, float value_scale, float* value_out,
                                int accumulate_value, float grad_coef, float* grad_flux_accum, int32_t* argmax_out,
                                const int* shift_dev, const float* offset_dev, void* stream);

/* The same prior with `jitter=True` (priors/patches/core.py:189-220; utils/torch.py:278-334): behind the norm and the roll
 * every patch row and every patch column is moved by a draw of its own.  With P the patch size of the handle (8 or 16),
 * `stride` the prior's stride in [1, P] and overlap = P - stride, along an axis of length n
 *   count = len(arange(overlap, n - stride - overlap, stride)),   pos_i = overlap + i stride + draw_i,
 * n_y = count(H), n_x = count(W), and patch (i, j) is rolled_normed[py_i : py_i + P, px_j : px_j + P].  jitter_y_dev /
 * jitter_x_dev: DEVICE arrays of n_y / n_x int32, the draws themselves (the reference draws x first), each in
 * [-overlap, overlap].  They live on the device and cannot be validated here: inside the kernels a draw is CLAMPED to that
 * range (the Python layer validates what it uploads), and the flux is read through a non-negative mod, so no value of a
 * draw reads outside the image.  An axis is safe when overlap + (count - 1) stride + overlap <= n - P: no draw can push a
 * patch outside (the reference has no such check and fails at random).
 * Two streaming kernels around the unchanged pass: the first writes the patches side by side,
 *   S[i P + a, j P + b] = n(flux[(py_i + a - shift_y) mod H, (px_j + b - shift_x) mod W]),
 * and zeroes an image G of the same shape; jd_gmm_prior_fwd_bwd runs on S ((n_y P, n_x P), stride P, no roll, identity
 * norm, the handle's patch norm), G = grad_coef d(sum v_patch)/dS; the second adds, per flux pixel with
 * (Y, X) = ((y + shift_y) mod H, (x + shift_x) mod W),
 *   n'(flux[y, x]) sum_{i: 0 <= Y - py_i < P} sum_{j: 0 <= X - px_j < P} G[i P + (Y - py_i), j P + (X - px_j)]
 * to grad_flux_accum, i ascending then j ascending, no atomics: run-to-run identical.  A pixel whose sum is exactly 0
 * (no patch covers it, or under a norm n' may be infinite) is not written.  S and G (about 4 x the image each at stride
 * P / 2) belong to the handle and grow on demand: after the first call for a shape nothing is allocated.
 * Value, value_scale, accumulate_value, grad_coef, marginalize, the image norm and the patch norm of the handle (left as
 * found) mean what they mean for jd_gmm_prior_fwd_bwd; argmax_out: one int32 per patch in order i n_x + j; shift_dev as
 * there.  With stride == P the result is that call's on the crop flux[:n_y P, :n_x P], bit for bit.  The WHOLE prior only
 * (no patch row shard, no band, no phases, no fused optimizer step); D = 64 and D = 256 handles.
 * JD_ERR_INVALID, nothing launched, the handle usable: a NULL gmm, flux, value_out or jitter array; n_y == 0 or n_x == 0;
 * an axis that is not safe; stride outside [1, P]; a staged image of 2^31 elements or more. */
int jd_gmm_prior_jitter_fwd_bwd(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                                const int* jitter_y_dev, const int* jitter_x_dev, int marginalize, float value_scale,
                                float* value_out, int accumulate_value, float grad_coef, float* grad_flux_accum,
                                int32_t* argmax_out, const int* shift_dev, void* stream);

/* The PRIOR IMAGE of one draw (priors/patches/core.py:123-151 `prior_image`; the reference's method cannot run as written,
 * this is the formula its lines state): what the mixture believes the flux looks like.  With N = n(flux) under the handle's
 * image norm, R0 = roll(N, (shift_y, shift_x)), the patch grid of jd_gmm_prior_fwd_bwd (n_y x n_x patches of P x P pixels,
 * P = 8 or 16 by the handle), m_ij the mean of patch (i, j) of R0 and k_ij the arg-max component of its mean-free pixels
 * (ALWAYS the max mode; -1 for a patch the `> -1e5` filter drops),
 *   R[Y, X]           = sum_{(i, j) covering (Y, X), k_ij >= 0} w[Y - i s, X - j s] (T[k_ij][Y - i s, X - j s] + m_ij),
 *   image_accum[y, x] = (accumulate ? += : =) scale * n^-1(R[(y + shift_y) mod H, (x + shift_x) mod W]),
 * w = get_pixel_weights((P, P), stride) (utils/numpy.py:54-79), patches added in ascending (i, j), 0 where no patch covers a
 * pixel (then n^-1(0)), n^-1 the norm's `inverse` (utils/norms.py) -- np.roll(reco, -shift) followed by norm.inverse.
 * patch_images: DEVICE table T of K * P * P floats (the caller's choice: the eigen-images of the covariances, the means, ...).
 * Averaging over n draws is n calls with accumulate = 1 (0 for the first) and scale = 1 / n.
 * The unchanged max-mode forward pass runs first, into an arg-max buffer of the handle; then two kernels (csrc/gmm_prior_image.hip):
 * the patch means of the rolled, normed image, and a gather per output pixel with the winners and means of a tile's patches
 * staged in LDS.  No atomics, a fixed order of the additions: two runs give the same bits.  No host synchronisation; the
 * work buffers belong to the handle and grow on demand: after the first call for a shape nothing is allocated.
 * shift_dev as for jd_gmm_prior_fwd_bwd.  D = 64 and D = 256 handles.
 * JD_ERR_INVALID, nothing launched, the handle usable: a NULL gmm, flux, patch_images or image_accum; an image smaller than a
 * patch; stride < 1 or stride >= P (the trapezoid's slope is 1 / overlap); a handle whose patch norm is the standardized
 * one (the formula adds back the mean only). */
int jd_gmm_prior_image(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                       const float* patch_images, float scale, float* image_accum, int accumulate,
                       const int* shift_dev, void* stream);

/* Diagnostics of the screened arg-max path, read without synchronisation from host-mapped memory the last block of a
 * pass writes: out[0..4] = {generation of the last finished pass, it fell back to the dense fp32 kernel (0 / 1), bucket
 * slots its surviving records used, patches it covered, gradient rows per patch the record buffer has room for now}.
 * The library uses the same numbers to double that room (4 -> 32) after a pass that ran out of it. */
int jd_gmm_screen_stats(const jd_gmm* gmm, int* out);
/* The shader clock the board holds INSIDE the screen kernel (a measurement tool of bench.py: the matrix roof the kernel
 * is priced against scales with it).  The first call arms the handle: its default screen launch then runs an instantiation
 * whose blocks leave s_memtime / s_memrealtime tick counts between their first and last instruction.  Later calls
 * synchronise the device, return the mean of 100 MHz x (shader ticks / reference ticks) over the blocks stamped since the
 * previous call (samples_out of them, at most 4096 per launch) and clear the stamps. */
int jd_gmm_screen_clock(jd_gmm* gmm, double* mhz_out, int* samples_out);

/* The same evaluation for ONE RANK OF A SHARDED PRIOR (joint fit over several GPUs; the
 * reference has no distributed code): instead of accumulating into the gradient image, the gradient of the shard's
 * patch rows is written as a compact band of the ROLLED frame,
 *   band_out[(Y - y_begin) * W + X] = grad_coef * d(sum_{patches in shard} v_patch)/d flux_rolled[Y, X],
 *   Y in [y_begin, y_end) = [patch_row_begin * stride, (patch_row_end - 1) * stride + 8)   (0 where no patch covers),
 * which the ranks exchange with ONE all-gather while the all-reduce of the likelihood gradient is in flight. */
int jd_gmm_prior_band_fwd_bwd(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y,
                              int shift_x, int patch_row_begin, int patch_row_end, int marginalize,
                              float value_scale, float* value_out, int accumulate_value, float grad_coef,
                              float* band_out, void* stream);
/* grad[(Y - shift_y) mod H, (X - shift_x) mod W] += sum_b bands[b * chunk_floats + (Y - y_begin[b]) * W + X] over the
 * bands with y_begin[b] <= Y < y_end[b], added in band order (identical on every rank).  `bands` is the device buffer an
 * all-gather of the per-rank bands produced; y_begin / y_end are HOST arrays of n_bands (<= 64) entries. */
int jd_add_rolled_bands(float* grad, int H, int W, int shift_y, int shift_x, const float* bands, size_t chunk_floats,
                        int n_bands, const int* y_begin, const int* y_end, void* stream);
/* The same sum followed at once by the optimizer step of jd_adam_step (sharded fits, where the prior's bands are the
 * last term of the gradient): every pixel takes g = step->grad_flux[pixel] + (the band sum above, same additions in the
 * same order) -- the gradient image itself is only read -- and the update of jd_adam_step with g: the bits of
 * jd_add_rolled_bands followed by jd_adam_step, one launch and one pass over the gradient image less.  Needs W % 4 == 0
 * and 16-byte aligned images (JD_ERR_INVALID otherwise: use the two calls).  step->addend is not supported here: a
 * non-null step->addend[0] returns JD_ERR_INVALID (use jd_add_rolled_bands + jd_adam_step_addends). */
int jd_add_rolled_bands_step(int H, int W, int shift_y, int shift_x, const float* bands, size_t chunk_floats, int n_bands,
                             const int* y_begin, const int* y_end, const jd_step* step, void* stream);

/* (Np, K) log-probabilities of explicit patches: GaussianMixtureModel.estimate_log_prob
 * (patches/gmm.py:262-281).  x: (n, D) device (D of the handle: 64 or 256), out: (n, K) device. */
int jd_gmm_estimate_log_prob(jd_gmm* gmm, const float* x, int n, float* out, void* stream);

/* FITTING A MIXTURE (csrc/gmm_fit.hip): the device half of one EM step of a full-covariance Gaussian mixture, as in
 * sklearn.mixture.GaussianMixture(covariance_type="full").  With d_nk = x_n - means[k], l_nk = const_k[k] -
 * |prec_chol[k]^T d_nk|^2 / 2, lse_n = logsumexp_k l_nk (max-shifted) and r_nk = exp(l_nk - lse_n), jd_gmm_fit_step
 * writes K + K D + K D D + 1 doubles to sums_out:
 *   [sum_n r_nk (K) | sum_n r_nk d_nk (K, D) | sum_n r_nk d_nk d_nk^T (K, D, D) | sum_n lse_n] .
 * The moments are about the means the call was given; the caller finishes the M-step on the host in float64.
 * x (n, D), means (K, D), prec_chol (K, D, D: UPPER TRIANGULAR factors P_k, row major; entries below the diagonal are
 * never read), const_k (K) = log w_k + log det P_k - D/2 log 2 pi and sums_out are DEVICE pointers, borrowed for the
 * call; x needs float alignment only, and its alignment changes no bit of the result.  The whitening runs on
 * v_mfma_f32_16x16x4_f32; the moments are accumulated in float64 (the second ones on v_mfma_f64_16x16x4_f64, from exact
 * products).  No atomics: blocks add into float64 partial sums of their own
 * and a second launch adds those in a fixed order, so two calls on the same input give the same bits.
 * The handle owns the partial sums: at most max_blocks sets of K (D D + D + 1) doubles, max_blocks = 0 selecting the
 * default, the number of compute units, lowered where the sets would exceed 8 GiB.  They are allocated by the first step
 * and whenever a step needs more sets than any before it; apart from that a step allocates nothing and never
 * synchronises.  Supported: D = 64 or 256, 1 <= K <= 1024, 1 <= n <= (2^31 - 1) / D.  Anything else, a null handle and
 * null pointers return JD_ERR_INVALID with a message and launch nothing.  jd_gmm_fit_destroy(NULL) is a no-op. */
typedef struct jd_gmm_fit jd_gmm_fit;
int jd_gmm_fit_create(int D, int K, int max_blocks, jd_gmm_fit** fit_out);
int jd_gmm_fit_destroy(jd_gmm_fit* fit);
int jd_gmm_fit_step(jd_gmm_fit* fit, const float* x, long long n, const float* means, const float* prec_chol,
                    const float* const_k, double* sums_out, void* stream);
/* The same sums for HARD assignments, r_nk = [labels[n] == k] (the k-means start of the fit): no whitening, the last
 * slot (sum lse) is 0, the layout, the float64 accumulation, the fixed order and the limits are those of jd_gmm_fit_step.
 * labels (n, int32, device) is only compared with k: a label outside [0, K) contributes to nothing. */
int jd_gmm_fit_step_labels(jd_gmm_fit* fit, const float* x, long long n, const float* means, const int* labels,
                           double* sums_out, void* stream);

/* K-MEANS ON PATCHES (csrc/kmeans.hip): one Lloyd step.  With the scores s_nk = |centres[k]|^2 - 2 x_n . centres[k]
 * (float32 products on v_mfma_f32_16x16x4_f32; |c|^2 summed in float64 and rounded once) jd_kmeans_step writes
 *   labels[n] = argmin_k s_nk, the lowest k on a tie, and -1 for a patch one of whose scores is not finite, and
 *   K + K D + 3 doubles to sums_out: [count_k (K) | sum of the patches of cluster k (K, D) | inertia | changed | unassigned],
 * inertia = sum_n max(|x_n|^2 + s_n,label, 0) evaluated in float64 for the chosen centre, changed = the number of patches
 * whose label differs from the value labels[n] held on entry, unassigned = the number of labels -1 (such patches are in no
 * sum).  x (n, D), centres (K, D), labels (n, read and written) and sums_out are DEVICE pointers, borrowed for the call;
 * float alignment is enough for x.  The cluster sums are accumulated in float64 (exact products on
 * v_mfma_f64_16x16x4_f64).  No atomics: blocks write partial sums of their own and a last launch adds them in block
 * order, so two calls on the same input give the same bits.  The handle owns the partial sums (at most max_blocks sets of
 * K (D + 1) + 3 doubles; 0 selects the default, twice the number of compute units), allocated by the first step and when a
 * step needs more sets than any before it; apart from that a step allocates nothing and never synchronises.
 * Supported: D = 64 or 256, 1 <= K <= 1024, 1 <= n <= (2^31 - 1) / D.  Anything else, a null handle and null pointers
 * return JD_ERR_INVALID with a message and launch nothing.  jd_kmeans_destroy(NULL) is a no-op. */
typedef struct jd_kmeans jd_kmeans;
int jd_kmeans_create(int D, int K, int max_blocks, jd_kmeans** kmeans_out);
int jd_kmeans_destroy(jd_kmeans* kmeans);
int jd_kmeans_step(jd_kmeans* kmeans, const float* x, long long n, const float* centres, int* labels, double* sums_out,
                   void* stream);

/* Element-wise priors: InverseGammaPrior (priors/core.py:207-226; kind 1: alpha, beta) and
 * ExponentialPrior (priors/core.py:308-326; kind 2: alpha).  value_out <- sum(v)/n + log_const;
 * grad_flux_accum += grad_coef * d value / d flux. */
int jd_elementwise_prior_fwd_bwd(int kind, const float* flux, size_t n, float alpha, float beta,
                                 float log_const, float* value_out, float grad_coef,
                                 float* grad_flux_accum, void* stream);
/* The same priors with `cycle_spin_subpix=True` (priors/core.py:220-221,321-322; utils/torch.py:31-38,122-143): the prior
 * is evaluated on s = K (*) flux, the 3 x 3 cross-correlation ("same", zero outside the (H, W) image) with
 * k[i][j] = wx(j - 1) * wy(i - 1), w(t) = 1 - |t - o| where |t - o| < 1 else 0 for the offsets o = x0, y0 in [-0.5, 0.5]
 * that the caller drew (x0 first); the weights are formed in the kernel in the reference's float32 operations.
 * value_out <- sum(v(s)) / (H W) + log_const;  grad_flux_accum += grad_coef * K^T v'(s) (NULL: value only).
 * One launch over 2-D tiles (flux tile + halo staged in LDS, one read-modify-write of the gradient per pixel, no atomics:
 * run-to-run identical) plus the fixed-order sum of the block partials.
 * offset_dev != NULL: device [2] = {x0, y0}, read by the kernel instead of the two by-value arguments (see
 * jd_gmm_prior_fwd_bwd: device-resident step scalars).  By-value offsets outside [-0.5, 0.5] or not finite, a kind other
 * than 1 / 2, a NULL flux or value_out and a non-positive shape return JD_ERR_INVALID. */
int jd_elementwise_prior_subpix_fwd_bwd(int kind, const float* flux, int H, int W, float alpha, float beta,
                                        float log_const, float x0, float y0, const float* offset_dev,
                                        float* value_out, float grad_coef, float* grad_flux_accum, void* stream);
/* SmoothnessPrior (priors/core.py:373-384): value_out <- -sum(flux * (K (*) flux)) for the kernel whose operator `khat`
 * jd_conv_psf_spectrum built for `plan` (the plan's (H, W) is the image; "same" zero-padded convolution, no division by
 * the number of pixels);  grad_flux_accum += grad_coef * (-2 K (*) flux) (NULL: value only) -- K is symmetric and odd-sized,
 * so the operator is its own adjoint.  Runs jd_conv_same into a scratch image of the library (grown on the first call of a
 * size: not inside a captured region) and one streaming launch behind it. */
int jd_smoothness_prior_fwd_bwd(jd_conv_plan* plan, const float* khat, const float* flux, float* value_out,
                                float grad_coef, float* grad_flux_accum, void* stream);

/* Parameter update -------------------------------------------------------------------------
 * flux = exp(theta) [* mask]   (SpatialFluxComponent.flux_upsampled, models/core.py:583-594);
 * use_log_flux == 0: flux = theta [* mask] (the parameter is the flux itself, no positivity). */
int jd_flux_from_theta(const float* theta, const float* mask, float* flux, size_t n, int use_log_flux, void* stream);

/* Flux components that SHARE one forward operator.  NPredModels.from_dataset_numpy (models/npred.py:279-295) builds the
 * model of every component of a dataset from the same exposure and -- unless `psf` is a dict -- the same PSF, and
 * NPredModels.evaluate (models/npred.py:241-261) adds clip(PSF * (flux_c x exposure), 0) over the components: with a
 * non-negative PSF, exposure and fluxes no term is ever clipped, so by linearity ONE convolution of (sum_c flux_c) x exposure
 * gives npred, and d loss / d flux_c is the same image for every c.  The host side (jolideco_amd/loss.py) then runs the
 * single-component launches between these two helpers:
 *   jd_sum_images:    out[i] = ((srcs[0][i] + srcs[1][i]) + ...)    n_srcs in [1, 4], host array of device pointers
 *   jd_copy_image_to: dsts[d][i] = src[i]                           n_dsts in [1, 4] */
int jd_sum_images(float* out, const float* const* srcs, int n_srcs, size_t n, void* stream);
int jd_copy_image_to(const float* src, float* const* dsts, int n_dsts, size_t n, void* stream);

/* Device-resident step scalars (see jd_gmm_prior_fwd_bwd): dst[0 .. n) <- host_row[0 .. n), read by ONE small block
 * straight from PINNED host memory (hipHostMalloc'ed, e.g. a torch tensor after pin_memory(): device-accessible) -- the
 * epoch's shifts and bias terms reach the device without a copy-engine hand-over on the stream.  The caller keeps the row
 * untouched until the launch has run (jolideco_amd/core.py StepScalars: a ring of rows guarded by events). */
int jd_step_scalars_fetch(const int32_t* host_row, int32_t* dst, int n, void* stream);

/* One torch.optim.Adam step (jolideco/core.py:39-42,229) on theta with the chain rule of
 * models/core.py:588-592 fused in: g_theta = grad_flux * flux_in.  Writes theta, exp_avg,
 * exp_avg_sq in place, writes flux_out = exp(theta_new) [* mask] (may alias flux_in or be a second
 * buffer so the caller can keep the pre-step flux for the loss trace, core.py:247) and zeroes
 * grad_flux when zero_grad != 0.  step_size = lr / (1 - beta1^t), bias2_sqrt = sqrt(1 - beta2^t),
 * one_minus_beta1 = 1 - beta1 and one_minus_beta2 = 1 - beta2 are computed by the caller in double
 * precision and rounded once, as torch does (fp32(1 - 0.999) != 1 - fp32(0.999)).
 * bias_dev != NULL: device [2] = {step_size, bias2_sqrt}, read by the kernel instead of the two by-value arguments (see
 * jd_gmm_prior_fwd_bwd: device-resident step scalars). */
int jd_adam_step(float* theta, const float* flux_in, float* flux_out, float* grad_flux, float* exp_avg,
                 float* exp_avg_sq, const float* mask, size_t n, float step_size, float beta1,
                 float beta2, float one_minus_beta1, float one_minus_beta2, float bias2_sqrt, float eps,
                 int zero_grad, int use_log_flux, const float* bias_dev, void* stream);
/* jd_adam_step on the gradient ((grad_flux + addends[0]) + addends[1]) + ... -- the leading non-null entries of the host
 * array addends[JD_ADDEND_MAX], device images of n floats (jd_npred_poisson_batch_addends_fwd_bwd); they are only read. */
int jd_adam_step_addends(float* theta, const float* flux_in, float* flux_out, float* grad_flux, float* exp_avg,
                         float* exp_avg_sq, const float* mask, size_t n, float step_size, float beta1,
                         float beta2, float one_minus_beta1, float one_minus_beta2, float bias2_sqrt, float eps,
                         int zero_grad, int use_log_flux, const float* bias_dev, const float* const* addends, void* stream);
/* jd_adam_step with use_log_flux = 0 for MANY small parameter vectors in ONE launch (the calibration parameters of the
 * datasets of a joint step, jolideco/core.py:197-204,229): tensor i (sizes[i] floats) takes its own step_size[i] /
 * bias2_sqrt[i] (its own step count, as torch.optim.Adam keeps one per parameter).  Host arrays of n_tensors <= 64
 * entries.  Same bits as n_tensors calls of jd_adam_step.  bias_dev != NULL: device [2 n_tensors], {step_size,
 * bias2_sqrt} of tensor i at [2 i], read by the kernel instead of the two host arrays (which may then be NULL). */
int jd_adam_step_multi(int n_tensors, float* const* theta, const float* const* grad, float* const* exp_avg,
                       float* const* exp_avg_sq, const int* sizes, const float* step_size, const float* bias2_sqrt,
                       float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                       const float* bias_dev, void* stream);
/* plain SGD (core.py:41): theta -= lr * grad_flux * flux_in, the update as ONE fused multiply-add (torch's add_(grad, alpha=-lr)) */
int jd_sgd_step(float* theta, const float* flux_in, float* flux_out, float* grad_flux,
                const float* mask, size_t n, float lr, int zero_grad, int use_log_flux, void* stream);

/* The optimizer step with the options of torch.optim.Adam / torch.optim.SGD (csrc/optimizer.hip; jolideco/core.py:39-42
 * hands `optimizer_kwargs` to them unchanged).  One kernel family and one launcher with jd_adam_step, jd_adam_step_addends
 * and jd_sgd_step, which are this entry with every option at its torch default ("off"): the library picks the kernel from
 * the options, and with none it is the plain float32 step, the same launch and the same bits.  The fused steps above know
 * no option.  Timed under JD_KERNEL_ADAM like every other step kernel.
 *   Adam: weight_decay      g += weight_decay * theta, before the moments
 *         decoupled_weight_decay != 0 (AdamW): theta *= 1 - lr * weight_decay instead, before the update
 *         amsgrad != 0      max_exp_avg_sq = max(max_exp_avg_sq, exp_avg_sq) takes exp_avg_sq's place in the denominator
 *         With any of the three the operations of a parameter run in double and every image is rounded once (the
 *         error against torch.optim in float64 is then that of the float32 images, whatever the operation order).
 *   SGD:  weight_decay      as above, one fused multiply-add -- SGD with options gives the bits of torch's float32 kernels
 *         momentum          buf = first_step ? g : momentum * buf + (1 - dampening) * g;  g = nesterov ? g + momentum * buf : buf
 *                           first_step: the first step in which the parameter has a gradient -- the buffer BECOMES the
 *                           gradient (weight decay included, no dampening) and is not read
 * The chain rule in front (g = grad_flux * flux_in; use_log_flux = 0: * mask) and flux_out = exp(theta) [* mask] behind are
 * those of jd_adam_step: under a mask the flux gradient of theta is 0, weight decay moves theta all the same, the flux
 * stays 0.  lr, weight_decay, momentum and dampening are doubles: 1 - lr * weight_decay and 1 - dampening are formed in
 * double and rounded once, as torch does with its Python floats. */
enum { JD_OPTIMIZER_ADAM = 0, JD_OPTIMIZER_SGD = 1 };
typedef struct {
  int kind;                  /* JD_OPTIMIZER_ADAM / JD_OPTIMIZER_SGD */
  float step_size, beta1, beta2, one_minus_beta1, one_minus_beta2, bias2_sqrt, eps; /* Adam: as jd_adam_step */
  double lr;                 /* SGD: the step; Adam: only in 1 - lr * weight_decay (step_size carries it otherwise) */
  double weight_decay;       /* >= 0 */
  double momentum, dampening; /* SGD; momentum >= 0 */
  int decoupled_weight_decay; /* Adam */
  int amsgrad;               /* Adam: needs max_exp_avg_sq */
  int nesterov;              /* SGD: needs momentum > 0 and dampening == 0 */
  int first_step;            /* SGD with momentum, see above (jd_optimizer_step_multi: per tensor, this one is not read) */
} jd_optimizer_options;
/* The images of jd_adam_step and the state images the options need: exp_avg, exp_avg_sq (Adam), max_exp_avg_sq (amsgrad),
 * momentum_buffer (SGD with momentum != 0); the others may be NULL and are not touched.  16-byte loads and stores where n
 * % 4 == 0 and every image is 16-byte aligned, pixel by pixel otherwise: the same bits.  bias_dev as in jd_adam_step (Adam).
 * JD_ERR_INVALID before anything is touched: a NULL required pointer, n == 0, a missing state image, an unknown kind, a
 * negative or non-finite lr / weight_decay / momentum, a non-finite dampening, nesterov without momentum or with
 * dampening, an Adam option with SGD or an SGD option with Adam. */
int jd_optimizer_step(float* theta, const float* flux_in, float* flux_out, float* grad_flux, float* exp_avg,
                      float* exp_avg_sq, float* max_exp_avg_sq, float* momentum_buffer, const float* mask, size_t n,
                      const jd_optimizer_options* options, int zero_grad, int use_log_flux, const float* bias_dev,
                      void* stream);
/* jd_optimizer_step with use_log_flux = 0 and no mask for MANY small parameter vectors in ONE launch (jd_adam_step_multi is
 * this entry for Adam with no option: the same kernel): host arrays of n_tensors <= 64 entries; tensor i takes
 * step_size[i] / bias2_sqrt[i] (Adam; or bias_dev, device [2 n_tensors]) and first_step[i] (SGD with momentum; NULL
 * otherwise).  State pointer arrays an option does not need may be NULL.  Same bits as n_tensors calls of
 * jd_optimizer_step; the same refusals, and n_tensors outside [1, 64]. */
int jd_optimizer_step_multi(int n_tensors, float* const* theta, const float* const* grad, float* const* exp_avg,
                            float* const* exp_avg_sq, float* const* max_exp_avg_sq, float* const* momentum_buffer,
                            const int* sizes, const float* step_size, const float* bias2_sqrt, const int* first_step,
                            const jd_optimizer_options* options, const float* bias_dev, void* stream);

/* Sparse point-source flux component (models/core.py:54-342, utils/torch.py:31-38) ------------------------------
 * A list of n sources: param_flux[i] = log(flux_i) when use_log_flux != 0, else flux_i; x_pos[i] / y_pos[i] pixel
 * coordinates (pixel centres at integers, x indexes columns, y rows -- the reference's component compares its `x_pos` with
 * the ROW index, models/core.py:198-223, so the Python layer passes its `y_pos` as x_pos here and its `x_pos` as y_pos).
 * All vectors: device, n floats.
 *
 * jd_sparse_render: flux_out (H, W) <- the rendered image.  EVERY pixel is written:
 *   flux_out[y, x] = sum_i (wx_i(x) * wy_i(y)) * f_i,   w(t) = 1 - |t - t0| where |t - t0| < 1, else 0,
 *   f_i = exp(param_flux[i]) or param_flux[i],
 * the weights in the reference's float32 operations one by one (no contraction), the sum over the sources that touch the
 * pixel in ascending index order, 0 where none does.  A source touches at most 2 x 2 pixels; one on an exactly integer
 * coordinate touches one column (row); one whose taps all lie outside the image contributes nothing.  Two launches (the
 * zero fill; one thread per (source, tap): the thread of the lowest source index on a pixel sums and stores it), no
 * atomics: run-to-run identical however many sources share a pixel.  Every tap is tested against every source:
 * O(n^2) work, for the hundreds to thousands of sources such a component holds.
 * Supported: 1 <= n <= jd_sparse_max_sources() (65536), 1 <= H, W <= 2^24; JD_ERR_INVALID beyond, and for null pointers. */
int jd_sparse_max_sources(void);
int jd_sparse_render(const float* param_flux, const float* x_pos, const float* y_pos, int n, int use_log_flux, int H,
                     int W, float* flux_out, void* stream);
/* The gradients of a loss with respect to the three vectors, given grad_flux_image = d loss / d flux_out (H, W): one
 * thread per source reads its <= 4 taps G and ASSIGNS (nothing is accumulated)
 *   grad_param[i] = c_i * sum wx wy G               (c_i = f_i for log flux, 1 for linear flux)
 *   grad_x[i]     = f_i * sum sign(x - x_i) wy G
 *   grad_y[i]     = f_i * sum wx sign(y - y_i) G
 * with sign(0) = 0, as torch.abs / torch.where differentiate: a source on an exactly integer coordinate gets an exactly
 * zero position gradient on that axis.  Taps outside the image are skipped; a source wholly outside gets three zeros.
 * Same limits as jd_sparse_render. */
int jd_sparse_backward(const float* param_flux, const float* x_pos, const float* y_pos, int n, int use_log_flux, int H,
                       int W, const float* grad_flux_image, float* grad_param, float* grad_x, float* grad_y,
                       void* stream);

/* Pyramid of the multi-scale prior (priors/patches/core.py:303-324) -----------------------------------------------
 * Per level l, f = 2^l, the reference blurs the running image with a sampled Gaussian ("same", zero padded, cumulative:
 * core.py:316-320, `convolve_fft_torch`), takes f x f means (core.py:322, `F.avg_pool2d`: ragged rows / columns are
 * dropped) and hands them to the inner prior; autograd runs the chain backwards.  `taps`: HOST array of the n_taps
 * (odd, <= 43) factors u of the kernel K = u u^T, passed to the kernels by value; n_taps = 1 with u = {1} is no blur.
 *
 * jd_multiscale_down (one launch): g_out (H, W) <- K (*) src (skipped when NULL), d_out (H / f, W / f) <- the f x f
 * means of it, dd_zero (same shape, optional) <- 0.  The loads read src rolled by (shift_y, shift_x), both reduced modulo
 * the shape: rolled[y, x] = src[(y - shift_y) mod H, (x - shift_x) mod W] (core.py:303-308, `cycle_spin`).  The means
 * are summed in a fixed order without atomics: run-to-run identical.
 *
 * jd_multiscale_up_adjoint (one launch): out <- K^T (*) (dg + replicate_f(dd) / f^2); dg (H, W) may be NULL (the last
 * level).  rolled = 0: out (H, W) is assigned.  rolled = 1: out is the gradient image of the un-rolled flux and
 * out[(y - shift_y) mod H, (x - shift_x) mod W] += the result at [y, x].  With value_out the launch also writes
 * value_out[0] = sum_i level_coefs[i] * level_values[i] (i < n_values <= JD_MULTISCALE_MAX_LEVELS; level_values: device,
 * level_coefs: host; float32, index order: core.py:324).  jd_multiscale_value: that sum alone (a forward-only call).
 *
 * JD_ERR_INVALID, before anything reaches a device: null pointers, f not in {1, 2, 4, 8, 16}, an even number of taps or
 * more than 43, an image smaller than f, shifts outside [0, H) x [0, W), g_out == src or out == dg. */
#define JD_MULTISCALE_MAX_LEVELS 5
int jd_multiscale_down(const float* src, int H, int W, int f, const float* taps, int n_taps, int shift_y, int shift_x,
                       float* g_out, float* d_out, float* dd_zero, void* stream);
int jd_multiscale_up_adjoint(const float* dg, const float* dd, int H, int W, int f, const float* taps, int n_taps,
                             float* out, int rolled, int shift_y, int shift_x, const float* level_values,
                             const float* level_coefs, int n_values, float* value_out, void* stream);
int jd_multiscale_value(const float* level_values, const float* level_coefs, int n_values, float* value_out, void* stream);

/* Kernel timers -----------------------------------------------------------------------------
 * New (the reference has no profiler hooks).  After jd_profile_enable(n) the
 * library brackets every launch of the kernels below with a hipEvent pair on the launch stream
 * (at most n pairs; further launches are not timed); jd_profile_read synchronises on the recorded
 * events and returns the summed duration and the number of timed launches of one kernel.
 * Calling jd_profile_enable again resets the counters. */
enum {
  JD_KERNEL_POISSON_FUSED = 0,   /* K3: clip + background + Poisson NLL + gradient */
  JD_KERNEL_GMM_FWD = 1,         /* K4: GMM patch log-likelihood, max / logsumexp over components (whole forward pass) */
  JD_KERNEL_GMM_BWD = 2,         /* K4b: per-patch gradient for the selected component(s) */
  JD_KERNEL_GMM_GATHER = 3,      /* K4c: deterministic overlap-add of the patch gradients; the two launches of
                                    jd_gmm_prior_image behind its forward pass (patch means + overlap-add of the table) */
  JD_KERNEL_PAD_MUL = 4,         /* K1 */
  JD_KERNEL_CMUL = 5,            /* K2 */
  JD_KERNEL_ADJOINT_EPILOGUE = 6,/* K5 */
  JD_KERNEL_ADAM = 7,            /* K6 */
  JD_KERNEL_FFT_R2C = 8,         /* rocFFT real forward transform (all its kernels) */
  JD_KERNEL_FFT_C2R = 9,         /* rocFFT real inverse transform (all its kernels) */
  JD_KERNEL_DIRECT_CONV = 10,    /* MFMA Toeplitz convolution / correlation (small PSFs) */
  JD_KERNEL_SEP_CONV = 11,       /* separable (low-rank PSF) convolution / correlation */
  JD_KERNEL_GMM_SCREEN = 12,     /* K4 screened arg-max, stage 1: fp16 MFMA screen with error bounds (inside GMM_FWD) */
  JD_KERNEL_GMM_SORT = 13,       /*   stage 2: counting sort of the surviving (patch, component) records (inside GMM_FWD) */
  JD_KERNEL_GMM_EXACT = 14,      /*   stage 3: exact fp32 MFMA evaluation of the survivors (inside GMM_FWD) */
  JD_KERNEL_GMM_STAGE = 15,      /*   stage 0: patches -> mean-subtracted fp16 fragments, norms, scales (inside GMM_FWD) */
  JD_KERNEL_SHIFT = 16,          /* calibration: bilinear sub-pixel shift and its transpose (+ shift gradient partial sums) */
  JD_KERNEL_POISSON_MIXED = 17,  /* K3 for components of different up-sampling factors: pool + clip + NLL + replicated gradient */
  JD_KERNEL_ELEMENTWISE_SUBPIX = 18, /* element-wise priors with sub-pixel cycle spin: stencil + value + adjoint stencil */
  JD_KERNEL_SMOOTHNESS = 19,     /* smoothness prior: sum f (K * f) and its gradient behind the convolution */
  JD_KERNEL_ELEMENTWISE_PRIOR = 20, /* element-wise priors (inverse-gamma, exponential): value + gradient */
  JD_KERNEL_SPARSE_RENDER = 21,  /* sparse component: zero fill + one thread per (source, tap), index-ordered sums */
  JD_KERNEL_SPARSE_BACKWARD = 22, /* sparse component: gradients of flux and positions from the <= 4 taps of a source */
  JD_KERNEL_MULTISCALE_DOWN = 23, /* multi-scale prior: blur + f x f means of one level */
  JD_KERNEL_MULTISCALE_UP = 24,  /* multi-scale prior: adjoint of both (replicate + correlate) */
  JD_KERNEL_COUNT = 25
};
int jd_profile_enable(int capacity);
int jd_profile_disable(void);
/* pause (1) / resume (0) the timers without resetting them: lets a caller time a sample of its steps */
int jd_profile_pause(int paused);
int jd_profile_read(int kernel, double* total_ms, long long* launches);
const char* jd_kernel_name(int kernel);
/* Sustained shader clock of the current device under a vector-ALU load on every CU, in MHz (new; a measurement aid:
 * MI355X boards hold different clocks under load, so a benchmark line should say which clock its times were taken at).
 * Runs a dependent-FMA kernel for about `milliseconds` on `stream`, stamped with s_memtime / s_memrealtime, and
 * SYNCHRONISES the stream. */
int jd_clock_probe(double milliseconds, double* mhz_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JOLIDECO_HIP_H */

"""Python handles over the C-ABI of libjolideco_hip.so and the autograd seams built on them.

`ConvPlan` / `GmmHandle` own the native handles; the `*Function` classes are the
`torch.autograd.Function` wrappers that sit where the reference calls ATen ops
(SURVEY.md section 8(b)).  Nothing in this module computes on the CPU: every method requires HIP
tensors and raises RuntimeError otherwise.
"""
import ctypes
import math
import weakref
from ctypes import c_float, c_int, c_void_p

import numpy as np
import torch

from . import _hip
from ._hip import check, ptr, ptr_array, stream_ptr

__all__ = [
    "ConvPlan",
    "GmmHandle",
    "GmmFitHandle",
    "KMeansHandle",
    "ConvSameFunction",
    "PoissonNLLFunction",
    "GMMPatchPriorFunction",
    "ElementwisePriorFunction",
    "SmoothnessPriorFunction",
    "stirling_mean",
    "require_hip_tensor",
    "band_rows",
    "add_rolled_bands",
]

POISSON_EPS = 1e-25  # jolideco/loss.py:36


def require_hip_tensor(t, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{name} must live on a HIP device: jolideco_amd has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def stirling_mean(counts):
    """mean([c>1] * (c log c - c + 0.5 log(2 pi c))): the flux-independent Stirling term of
    nn.PoissonNLLLoss(full=True) (jolideco/loss.py:35-37), computed once per dataset in float64."""
    c = np.asarray(counts, dtype=np.float64)
    term = np.zeros_like(c)
    m = c > 1
    term[m] = c[m] * np.log(c[m]) - c[m] + 0.5 * np.log(2 * np.pi * c[m])
    return float(term.mean())


CONV_MODES = {"auto": 0, "fft-exact": 1, "fft": 2, "direct": 3, "separable": 4}  # JD_CONV_MODE_* (jolideco_hip.h)
CONV_METHOD_NAMES = {0: "fft", 1: "direct", 2: "separable"}  # jd_conv_plan_method


def psf_separable_rank(psf, tol=0.0):
    """Number of outer products (1..3) that reproduce a host PSF array to a few fp32 ulps, 0 if it is not
    that low-rank (jd_psf_separable_rank).  A sampled Gaussian is 1."""
    import numpy as np

    psf = np.ascontiguousarray(psf, dtype=np.float32)
    if psf.ndim != 2:
        raise ValueError(f"psf must be two dimensional, got shape {psf.shape}")
    return int(_hip.lib().jd_psf_separable_rank(psf.ctypes.data, psf.shape[0], psf.shape[1], float(tol)))


def default_conv_method():
    """Convolution method used when none is requested: "auto" -- the separable kernels when the PSF is a sum of at most
    three outer products; else the MFMA direct kernel up to 17 taps (up to 33 on images below a megapixel or where the
    native FFT sizes do not fit); else the FFT path (native transforms where the sizes allow, rocFFT otherwise) -- unless
    JOLIDECO_CONV_METHOD overrides it.  "general" = "auto" without the low-rank test (every PSF as a general kernel: what
    an instrument PSF that is no short sum of outer products gets; `bench.py`'s `general_psf` run)."""
    import os

    method = os.environ.get("JOLIDECO_CONV_METHOD", "auto")
    if method not in CONV_MODES and method != "general":
        raise ValueError(f"JOLIDECO_CONV_METHOD={method!r}, must be one of {sorted(CONV_MODES) + ['general']}")
    return method


def _forget_operator(address):
    try:
        _hip.lib().jd_conv_operator_forget(address)
    except Exception:  # interpreter shutdown: the library may be gone
        pass


class ConvPlan:
    """'same'-convolution plan for one (H, W, kh, kw) geometry (jd_conv_plan).

    ``method``: "auto" | "fft" (rocFFT, fast padded grid) | "fft-exact" (rocFFT on the reference's
    (H+kh-1, W+kw-1) grid) | "direct" (MFMA Toeplitz kernel, PSFs up to 33x33) | "separable" (row + column
    pass for low-rank PSFs, `psf_separable_rank`; `psf_spectrum` raises for a PSF that is not)."""

    _cache = {}

    def __init__(self, H, W, kh, kw, device, exact_shape=False, method=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ConvPlan needs a HIP device (no CPU fallback)")
        if method is None:
            method = "fft-exact" if exact_shape else default_conv_method()
        if method == "general":  # (the low-rank test is the caller's: a plan asked for by size alone is "auto")
            method = "auto"
        if method not in CONV_MODES:
            raise ValueError(f"unknown convolution method {method!r}, must be one of {sorted(CONV_MODES)}")
        handle = c_void_p()
        with torch.cuda.device(self.device):
            check(_hip.lib().jd_conv_plan_create(H, W, kh, kw, CONV_MODES[method], ctypes.byref(handle)))
        self._handle = handle
        shape = (c_int * 6)()
        check(_hip.lib().jd_conv_plan_shape(self._handle, shape))
        self.H, self.W, self.Hp, self.Wp, self.oy, self.ox = (int(v) for v in shape)
        self.kh, self.kw = kh, kw
        self.spectrum_size = int(_hip.lib().jd_conv_plan_spectrum_size(self._handle))
        self.method = CONV_METHOD_NAMES[_hip.lib().jd_conv_plan_method(self._handle)]

    @classmethod
    def get(cls, H, W, kh, kw, device, exact_shape=False, method=None):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if method is None:
            method = "fft-exact" if exact_shape else default_conv_method()
        if method == "general":
            method = "auto"
        key = (str(device), H, W, kh, kw, method)
        if key not in cls._cache:
            cls._cache[key] = cls(H, W, kh, kw, device, method=method)
        return cls._cache[key]

    @classmethod
    def clear_cache(cls):
        for plan in cls._cache.values():
            plan.close()
        cls._cache.clear()

    def close(self):
        if self._handle is not None:
            _hip.lib().jd_conv_plan_destroy(self._handle)
            self._handle = None

    @property
    def native_fft(self):
        """True when an "fft" plan runs on the hand-written transforms of csrc/fftnative.hip (no padded grid) instead of
        rocFFT (padded sizes 2^a * {1, 3, 9} up to 9216 columns x 4608 row pairs; any H, W since round 5; option JD_FFT_NATIVE=0 switches it off)."""
        return self.method == "fft" and (self.Hp, self.Wp) == (self.H, self.W)

    def takes_walk(self, n_datasets=1):
        """True when a launch over ``n_datasets`` datasets runs on the strip-walk kernels (jd_conv_plan_takes_walk)."""
        return bool(_hip.lib().jd_conv_plan_takes_walk(self._handle, int(n_datasets)))

    ROW_SCHEDULES = ("generic-large", "2304", "4608", "1152", "generic-small", "tiny", "generic-huge")  # row_schedule of csrc/fftnative.hip

    def step_route(self, upsampling=1, n_datasets=1):
        """The kernels a likelihood step of ``n_datasets`` datasets with this up-sampling factor launches
        (jd_conv_plan_step_route): dict of ``Nx``, ``Ny``, ``rows_fwd`` / ``rows_pooled`` (a name of `ROW_SCHEDULES` or None),
        ``pooled_supported``, ``pooled_column_io``, ``batched`` (0 per-dataset calls, 1 launches over all datasets, 2 FFT
        launches per dataset with a common tail) and ``shift_bwd_rows`` (R of the four-pixel kernel, 0: scalar kernels)."""
        out = (ctypes.c_int32 * 8)()
        check(_hip.lib().jd_conv_plan_step_route(self._handle, int(upsampling), int(n_datasets), out))
        name = lambda i: self.ROW_SCHEDULES[i] if i >= 0 else None  # noqa: E731
        return {
            "Nx": int(out[0]), "Ny": int(out[1]), "rows_fwd": name(out[2]), "rows_pooled": name(out[3]),
            "pooled_supported": bool(out[4]), "pooled_column_io": bool(out[5]), "batched": int(out[6]),
            "shift_bwd_rows": int(out[7]),
        }

    def fft_route(self, n_datasets=1):
        """The kernels a plain convolution, its adjoint and the un-up-sampled likelihood step launch on a native FFT plan
        (jd_conv_plan_fft_route; an error for any other plan): dict of ``Nx``, ``Ny``, ``col_lanes`` (threads per column),
        ``col_block`` (columns per block launched), ``col_static`` (1: a compile-time entry of the column table, 0: the
        generic kernel), ``rows_fwd`` (name of `ROW_SCHEDULES` of a forward-row launch over ``n_datasets`` datasets) and
        ``rows_inv`` (of the single-image inverse-row launch)."""
        out = (ctypes.c_int32 * 8)()
        check(_hip.lib().jd_conv_plan_fft_route(self._handle, int(n_datasets), out))
        return {
            "Nx": int(out[0]), "Ny": int(out[1]), "col_lanes": int(out[2]), "col_block": int(out[3]),
            "col_static": int(out[4]), "rows_fwd": self.ROW_SCHEDULES[out[5]], "rows_inv": self.ROW_SCHEDULES[out[6]],
        }

    def direct_kernel(self):
        """The instantiation of the MFMA Toeplitz kernel a "direct" plan launches (jd_conv_plan_direct_kernel): dict of
        ``KC`` (fp32: 16 .. 48, split: 32 or 64), ``split`` (the split-fp16 kernel, not the fp32 one) and ``vec_fwd`` /
        ``vec_adj`` (the forward convolution / the adjoint stages 16-byte chunks when its images are 16-byte aligned)."""
        out = (ctypes.c_int32 * 4)()
        check(_hip.lib().jd_conv_plan_direct_kernel(self._handle, out))
        return {"KC": int(out[0]), "split": bool(out[1]), "vec_fwd": bool(out[2]), "vec_adj": bool(out[3])}

    # --- kernel spectrum (once per dataset and component) -----------------------------------
    def psf_spectrum(self, psf, out=None):
        """The kernel operator of `psf` for this plan (jd_conv_psf_spectrum).  Operator buffers are immutable: to change
        the PSF of an existing buffer build the new operator INTO it (``out=``), which re-registers the address; an
        in-place copy of another operator's bytes is reported by the next library call."""
        psf = require_hip_tensor(psf, "psf")
        if tuple(psf.shape[-2:]) != (self.kh, self.kw):
            raise ValueError(f"psf shape {tuple(psf.shape)} does not match the plan ({self.kh}, {self.kw})")
        if out is not None:
            out = require_hip_tensor(out, "out")
            if out.numel() != 2 * self.spectrum_size or not out.is_contiguous():
                raise ValueError("out must be a contiguous operator buffer of this plan")
            check(_hip.lib().jd_conv_psf_spectrum(self._handle, ptr(psf), ptr(out), stream_ptr(psf.device)))
            return out
        khat = torch.empty(2 * self.spectrum_size, dtype=torch.float32, device=psf.device)
        check(_hip.lib().jd_conv_psf_spectrum(self._handle, ptr(psf), ptr(khat), stream_ptr(psf.device)))
        if self.method == "separable":
            # the library keeps what it knows about the operator (rank, support of its taps) by device address: the entry
            # goes with this tensor, so that a later allocation at the same address is an unknown buffer again (a view
            # that outlives the tensor is then unknown too: it takes the general kernels, never a wrong one)
            weakref.finalize(khat, _forget_operator, khat.data_ptr())
        return khat

    def walk_frame(self, khat):
        """17 / 33: the frame the strip-walk kernels run this operator in, 0: not theirs (jd_conv_operator_walk_frame)."""
        return int(_hip.lib().jd_conv_operator_walk_frame(self._handle, ptr(khat)))

    def _check_image(self, image, name):
        image = require_hip_tensor(image, name)
        if tuple(image.shape[-2:]) != (self.H, self.W) or image.numel() != self.H * self.W:
            raise ValueError(f"{name} shape {tuple(image.shape)} does not match the plan ({self.H}, {self.W})")
        return image

    def conv_same(self, image, scale, khat):
        image = self._check_image(image, "image")
        if scale is not None:
            scale = self._check_image(scale, "scale")
        out = torch.empty_like(image)
        check(_hip.lib().jd_conv_same(self._handle, ptr(image), ptr(scale), ptr(khat), ptr(out), stream_ptr(image.device)))
        return out

    def conv_same_adjoint(self, grad_out, scale, khat, grad_image=None, accumulate=False):
        grad_out = self._check_image(grad_out, "grad_out")
        if grad_image is None:
            grad_image = torch.empty_like(grad_out)
            accumulate = False
        check(
            _hip.lib().jd_conv_same_adjoint(
                self._handle, ptr(grad_out), ptr(scale), ptr(khat), ptr(grad_image), int(accumulate),
                stream_ptr(grad_out.device),
            )
        )
        return grad_image

    def npred_poisson_fwd_bwd(
        self, fluxes, exposures, khats, background, counts, stirling, loss_out, grads=None, accumulate=False,
        grad_scale=1.0, npred_out=None, eps=POISSON_EPS, upsampling=1, calibration=None,
    ):
        """Fused forward model + Poisson NLL (+ gradient) of one dataset; see include/jolideco_hip.h."""
        n = len(fluxes)
        if not (len(exposures) == len(khats) == n):
            raise ValueError("fluxes, exposures and khats must have the same length")
        for f in fluxes:
            self._check_image(f, "flux")
        if calibration is not None:
            # (shift_xy | None, log_background_norm, grad_shift_xy | None, grad_log_background_norm | None)
            shift, log_norm, grad_shift, grad_log_norm = calibration
            check(
                _hip.lib().jd_npred_poisson_calibrated_fwd_bwd(
                    self._handle, n, ptr_array(fluxes), ptr_array(exposures), ptr_array(khats), ptr(background),
                    ptr(counts), c_float(stirling), c_float(eps), ptr(loss_out),
                    ptr_array(grads) if grads is not None else None, int(accumulate), c_float(grad_scale),
                    ptr(npred_out), int(upsampling), ptr(shift), ptr(log_norm), ptr(grad_shift), ptr(grad_log_norm),
                    stream_ptr(background.device),
                )
            )
            return
        check(
            _hip.lib().jd_npred_poisson_fwd_bwd(
                self._handle, n, ptr_array(fluxes), ptr_array(exposures), ptr_array(khats), ptr(background),
                ptr(counts), c_float(stirling), c_float(eps), ptr(loss_out),
                ptr_array(grads) if grads is not None else None, int(accumulate), c_float(grad_scale),
                ptr(npred_out), int(upsampling), stream_ptr(background.device),
            )
        )

    @staticmethod
    def npred_poisson_mixed_fwd_bwd(
        plans, upsamplings, fluxes, exposures, khats, background, counts, stirling, loss_out, grads=None,
        accumulate=False, grad_scale=1.0, npred_out=None, eps=POISSON_EPS,
    ):
        """Fused forward model + Poisson NLL (+ gradient) of one dataset whose flux components live on grids of
        different up-sampling factors: ``plans[c]`` / ``upsamplings[c]`` are the plan and the factor of component c
        (jd_npred_poisson_mixed_fwd_bwd, include/jolideco_hip.h)."""
        n = len(plans)
        if not (len(upsamplings) == len(fluxes) == len(exposures) == len(khats) == n):
            raise ValueError("plans, upsamplings, fluxes, exposures and khats must have the same length")
        if grads is not None and len(grads) != n:
            raise ValueError("one gradient image per flux component")
        for plan, f in zip(plans, fluxes):
            plan._check_image(f, "flux")
        handles = (c_void_p * n)(*[plan._handle.value for plan in plans])
        factors = (c_int * n)(*[int(u) for u in upsamplings])
        check(
            _hip.lib().jd_npred_poisson_mixed_fwd_bwd(
                handles, n, ptr_array(fluxes), ptr_array(exposures), ptr_array(khats), ptr(background), ptr(counts),
                c_float(stirling), c_float(eps), ptr(loss_out), ptr_array(grads) if grads is not None else None,
                int(accumulate), c_float(grad_scale), ptr(npred_out), factors, stream_ptr(background.device),
            )
        )

    MAX_BATCH = 16  # SEP_MAX_BATCH of csrc/kernels.h
    MAX_BATCH_COMPONENTS = 4  # SEP_BATCH_MAX_COMP

    def npred_poisson_batch_fwd_bwd(self, flux, exposures, khats, backgrounds, counts, stirlings, loss_outs, grad=None,
                                    accumulate=False, grad_scale=1.0, eps=POISSON_EPS, addends=None, side_stream=None):
        """All datasets of a joint step at once (separable plan shared by every dataset and component): one launch for
        the forward models + Poisson passes, one for the losses, one adjoint launch per flux component
        (jd_npred_poisson_batch_multi_fwd_bwd).  Same numbers as the per-dataset calls with ``accumulate`` from the
        second dataset on.

        One component: ``flux`` / ``grad`` are tensors and ``exposures`` / ``khats`` lists of per-dataset tensors.
        Several components: ``flux`` / ``grad`` are lists of tensors and ``exposures[d]`` / ``khats[d]`` lists with one
        tensor per component.

        ``addends`` (one component, one call's worth of datasets): images the library MAY write the adjoints of the
        datasets of the second PSF frame into, one image each, instead of adding them to ``grad`` -- on ``side_stream``
        (a `torch.cuda.Stream`, optional) beside the adjoint launch of the first frame (jd_npred_poisson_batch_addends_fwd_bwd).
        Returns how many of them it wrote: the caller owes ``grad + addends[0] + addends[1] ...`` (0: ``grad`` is complete)."""
        n = len(exposures)
        if not (len(khats) == len(backgrounds) == len(counts) == len(stirlings) == len(loss_outs) == n):
            raise ValueError("all per-dataset lists must have the same length")
        single = torch.is_tensor(flux)
        fluxes = [flux] if single else list(flux)
        grads = None if grad is None else ([grad] if single else list(grad))
        if single:
            exposures, khats = [[e] for e in exposures], [[k] for k in khats]
        n_comp = len(fluxes)
        if not 1 <= n_comp <= self.MAX_BATCH_COMPONENTS:
            raise ValueError(f"{n_comp} flux components: the batched joint step takes 1 to {self.MAX_BATCH_COMPONENTS}")
        if any(len(e) != n_comp for e in exposures) or any(len(k) != n_comp for k in khats):
            raise ValueError("every dataset needs one exposure and one operator per flux component")
        if grads is not None and len(grads) != n_comp:
            raise ValueError("one gradient image per flux component")
        for f in fluxes:
            self._check_image(f, "flux")
        if addends and single and grads is not None and n <= self.MAX_BATCH and not accumulate:
            for image in addends:
                self._check_image(image, "addend")
            used = c_int(0)
            images = list(addends)[: _hip.ADDEND_MAX]
            images += [None] * (_hip.ADDEND_MAX - len(images))
            stirling_arr = (c_float * n)(*[float(v) for v in stirlings])
            check(
                _hip.lib().jd_npred_poisson_batch_addends_fwd_bwd(
                    self._handle, n, ptr(fluxes[0]), ptr_array([e[0] for e in exposures]), ptr_array([k[0] for k in khats]),
                    ptr_array(backgrounds), ptr_array(counts), stirling_arr, c_float(eps), ptr_array(loss_outs), ptr(grads[0]),
                    0, c_float(grad_scale), ptr_array(images),
                    None if side_stream is None else c_void_p(side_stream.cuda_stream), ctypes.byref(used),
                    stream_ptr(fluxes[0].device),
                )
            )
            return used.value
        for start in range(0, n, self.MAX_BATCH):
            sl = slice(start, min(n, start + self.MAX_BATCH))
            m = sl.stop - sl.start
            stirling_arr = (c_float * m)(*[float(v) for v in stirlings[sl]])
            check(
                _hip.lib().jd_npred_poisson_batch_multi_fwd_bwd(
                    self._handle, m, n_comp, ptr_array(fluxes), ptr_array([e for es in exposures[sl] for e in es]),
                    ptr_array([k for ks in khats[sl] for k in ks]), ptr_array(backgrounds[sl]), ptr_array(counts[sl]),
                    stirling_arr, c_float(eps), ptr_array(loss_outs[sl]), None if grads is None else ptr_array(grads),
                    int(accumulate or start > 0), c_float(grad_scale), stream_ptr(fluxes[0].device),
                )
            )
        return 0

    def npred_poisson_calibrated_batch_fwd_bwd(self, flux, exposures, khats, backgrounds, counts, stirlings, loss_outs,
                                               calibrations, upsampling=1, grad=None, accumulate=False, grad_scale=1.0,
                                               eps=POISSON_EPS):
        """All datasets of a joint step of ONE flux component with per-dataset calibrations and / or up-sampling
        (jd_npred_poisson_calibrated_batch_fwd_bwd): the batched form of `npred_poisson_fwd_bwd(..., calibration=...)`
        per dataset with ``accumulate`` from the second dataset on -- same numbers.
        ``calibrations``: per dataset None or (shift_xy | None, log_background_norm | None, grad_shift_xy | None,
        grad_log_background_norm | None)."""
        n = len(exposures)
        if not (len(khats) == len(backgrounds) == len(counts) == len(stirlings) == len(loss_outs) == len(calibrations) == n):
            raise ValueError("all per-dataset lists must have the same length")
        self._check_image(flux, "flux")
        cals = [c if c is not None else (None, None, None, None) for c in calibrations]
        for start in range(0, n, self.MAX_BATCH):
            sl = slice(start, min(n, start + self.MAX_BATCH))
            m = sl.stop - sl.start
            stirling_arr = (c_float * m)(*[float(v) for v in stirlings[sl]])
            check(
                _hip.lib().jd_npred_poisson_calibrated_batch_fwd_bwd(
                    self._handle, m, ptr(flux), ptr_array(exposures[sl]), ptr_array(khats[sl]), ptr_array(backgrounds[sl]),
                    ptr_array(counts[sl]), stirling_arr, c_float(eps), ptr_array(loss_outs[sl]), ptr(grad),
                    int(accumulate or start > 0), c_float(grad_scale), int(upsampling),
                    ptr_array([c[0] for c in cals[sl]]), ptr_array([c[1] for c in cals[sl]]),
                    ptr_array([c[2] for c in cals[sl]]), ptr_array([c[3] for c in cals[sl]]), stream_ptr(flux.device),
                )
            )


class DeviceShifts:
    """Cycle-spin shifts of one prior evaluation held in DEVICE memory: ``dev`` = int32 tensor [shift_y mod H, shift_x mod W]
    the kernels read (jd_gmm_prior_fwd_bwd: device-resident step scalars), ``host`` = the same pair as the host drew it.
    For a sub-pixel cycle spin ``dev`` is a float32 view of the slot holding [x0, y0] (jd_elementwise_prior_subpix_fwd_bwd)."""

    __slots__ = ("dev", "host")

    def __init__(self, dev, host):
        self.dev, self.host = dev, host


class JitterRing:
    """The draws of a jittered patch grid on their way to the device without a host synchronisation: a ring of pinned host
    rows and device rows (as `StepScalars` does for the step scalars).  `upload` fills the next row, enqueues a non-blocking
    copy on the current stream and returns the two device views; the caller records the row's event behind the launch that
    reads them (`done`), and a row is reused only after that event -- RING evaluations later, so the wait is idle."""

    RING = 8

    def __init__(self, device):
        self.device = torch.device(device)
        self.host, self.dev, self.events = [None] * self.RING, [None] * self.RING, [None] * self.RING
        self.used = [False] * self.RING
        self.slot = 0

    def upload(self, jitter_y, jitter_x):
        """(device int32 [n_y], device int32 [n_x], slot) of two host int tensors"""
        n_y, n_x = int(jitter_y.numel()), int(jitter_x.numel())
        slot, n = self.slot, n_y + n_x
        if self.used[slot]:
            self.events[slot].synchronize()
            self.used[slot] = False
        if self.host[slot] is None or self.host[slot].numel() < n:
            size = max(256, 2 * n)
            self.host[slot] = torch.empty(size, dtype=torch.int32).pin_memory()
            self.dev[slot] = torch.empty(size, dtype=torch.int32, device=self.device)
            self.events[slot] = torch.cuda.Event()
        host, dev = self.host[slot], self.dev[slot]
        host[:n_y].copy_(jitter_y)
        host[n_y:n].copy_(jitter_x)
        dev[:n].copy_(host[:n], non_blocking=True)
        self.slot = (slot + 1) % self.RING
        return dev[:n_y], dev[n_y:n], slot

    def done(self, slot):
        self.events[slot].record()
        self.used[slot] = True

    def send(self, draws, counts, overlap):
        """(device jitter_y, device jitter_x, slot) of the ``draws`` = (jitter_y, jitter_x) of a grid of ``counts`` =
        (n_y, n_x).  Host sequences or tensors are validated (integer, the counts, in [-overlap, overlap]) and uploaded:
        `done(slot)` behind the launch that reads them.  int32 tensors on the ring's device go as they are, with slot None
        (nothing in them can be validated without a synchronisation: the kernels clamp)."""
        names = ("jitter_y", "jitter_x")
        on_device = [isinstance(j, torch.Tensor) and j.device.type == "cuda" for j in draws]
        if all(on_device):
            for name, j, n in zip(names, draws, counts):
                if j.dtype != torch.int32 or not j.is_contiguous() or j.numel() != n or j.device != self.device:
                    raise ValueError(f"{name} on the device must be a contiguous int32 tensor of {n} draws on {self.device}")
            return draws[0], draws[1], None
        if any(on_device):
            raise ValueError("jitter_y and jitter_x must both be on the host or both on the device")
        draws = [torch.as_tensor(j).reshape(-1) for j in draws]
        for name, j, n in zip(names, draws, counts):
            if j.dtype not in (torch.int32, torch.int64) or j.numel() != n:
                raise ValueError(f"{name} must hold {n} integer draws (the image's patch grid at this stride), got "
                                 f"{j.numel()} of {j.dtype}")
            if n and (int(j.min()) < -overlap or int(j.max()) > overlap):
                raise ValueError(f"{name} has a draw outside [-{overlap}, {overlap}]")
        with torch.cuda.device(self.device):
            return self.upload(*draws)


def jitter_counts(shape, patch, stride):
    """(n_y, n_x) of the jittered patch grid (`utils.torch.jitter_grid`; raises ValueError for an unsafe shape)"""
    from .utils.torch import jitter_grid

    base_y, base_x = jitter_grid(shape, (patch, patch), stride)
    return int(base_y.numel()), int(base_x.numel())


class GmmHandle:
    """GMM constants in MFMA fragment order on the device (jd_gmm)."""

    def __init__(self, precisions_cholesky, means_precisions_cholesky, log_det_cholesky, log_weights,
                 pixel_weights, device, const_float64=None):
        """``const_float64``: the per-component constants -D/2 log(2 pi) + log|P_k| + log pi_k evaluated in float64 (K,);
        what the float32 constants below lose of them goes to the library as well (jd_gmm_set_const_residual) and
        enters the passes under the standardized patch norm, whose values are small differences of large terms."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GmmHandle needs a HIP device (no CPU fallback)")
        pc = np.ascontiguousarray(precisions_cholesky, dtype=np.float32)
        mp = np.ascontiguousarray(means_precisions_cholesky, dtype=np.float32)
        K, D, _ = pc.shape
        # const_k = -0.5 * D * log(2 pi) + log|P_k| + log pi_k   (patches/gmm.py:276-281)
        two_pi_log = np.float32(np.log(np.float32(2 * np.pi)))
        const_k = (
            np.float32(-0.5) * (np.float32(D) * two_pi_log)
            + np.asarray(log_det_cholesky, dtype=np.float32)
            + np.asarray(log_weights, dtype=np.float32)
        ).astype(np.float32)
        pw = np.ascontiguousarray(np.asarray(pixel_weights, dtype=np.float32).reshape(-1))
        self.K, self.D = K, D
        handle = c_void_p()
        as_fp = lambda a: a.ctypes.data_as(ctypes.POINTER(c_float))  # noqa: E731
        with torch.cuda.device(self.device):
            check(_hip.lib().jd_gmm_create(K, D, as_fp(pc), as_fp(mp), as_fp(const_k), as_fp(pw), ctypes.byref(handle)))
        self._handle = handle
        self._jitter_ring = None  # (`JitterRing`, made by the first jittered evaluation)
        self._prior_table = None  # (`prior_image_table`: the host values and their device copy)
        if const_float64 is not None:
            residual = np.ascontiguousarray(np.asarray(const_float64, dtype=np.float64) - const_k.astype(np.float64), dtype=np.float32)
            if residual.shape != (K,):
                raise ValueError(f"const_float64 must hold one value per component, got shape {residual.shape}")
            with torch.cuda.device(self.device):
                check(_hip.lib().jd_gmm_set_const_residual(handle, as_fp(residual)))

    def close(self):
        if self._handle is not None:
            _hip.lib().jd_gmm_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_image_norm(self, norm):
        """Hand the image norm of the NEXT prior call to the library (jd_gmm_set_image_norm).  Priors with different norms
        may share this handle (`GaussianMixtureModel.handle` caches one per device), so every prior call sets it anew;
        ``norm``: an `ImageNorm` with a device kind, or None = identity."""
        kind, p0, p1 = (0, 0.0, 0.0) if norm is None else norm.device_params()
        if kind is None:
            raise NotImplementedError(f"image norm {type(norm).__name__} has no HIP kernel")
        data = _hip.ImageNormStruct(int(kind), float(p0), float(p1))
        check(_hip.lib().jd_gmm_set_image_norm(self._handle, ctypes.byref(data)))

    def set_patch_norm(self, patch_norm):
        """Hand the patch norm of the NEXT prior call to the library (jd_gmm_set_patch_norm); like the image norm it is a
        state of the shared handle, so every prior call sets it anew.  ``patch_norm``: a `PatchNorm` with a device kind, or
        None = subtract-mean."""
        kind = 0 if patch_norm is None else patch_norm.device_kind
        if kind is None:
            raise NotImplementedError(f"patch norm {type(patch_norm).__name__} has no HIP kernel")
        check(_hip.lib().jd_gmm_set_patch_norm(self._handle, int(kind)))

    def prior_fwd_bwd(self, flux, stride, shifts, value_out, value_scale, grad=None, grad_coef=0.0,
                      marginalize=False, patch_rows=(0, -1), accumulate_value=False, argmax_out=None, band_out=None, phases=3,
                      norm=None, patch_norm=None, subpix=None, jitter=None):
        """``band_out``: instead of accumulating into ``grad``, write the gradient of the patch rows ``patch_rows`` as the
        band of the rolled frame they cover (jd_gmm_prior_band_fwd_bwd; `band_rows` gives its extent).
        ``norm``: the prior's image norm (None = identity); the gradient is the one with respect to the raw flux.
        ``patch_norm``: the prior's patch norm (None = subtract-mean).
        ``subpix``: the offsets (x0, y0) of a sub-pixel cycle spin -- or a `DeviceShifts` whose ``dev`` holds them as two
        float32 in device memory -- applied behind the roll (jd_gmm_prior_subpix_fwd_bwd): the whole prior only.
        ``jitter``: the draws (jitter_y, jitter_x) of a jittered patch grid (jd_gmm_prior_jitter_fwd_bwd), one per patch row
        and one per patch column of `utils.torch.jitter_grid`, each in [-overlap, overlap]: host sequences or tensors --
        validated here, sent through a pinned ring without a host synchronisation -- or int32 tensors on the flux's device,
        which the kernels read as they are (nothing can be validated without a synchronisation: they clamp).  The whole prior
        only; excludes ``subpix``.  An unsafe shape raises ValueError."""
        if isinstance(shifts, DeviceShifts) and band_out is not None:
            raise ValueError("device-resident shifts are not available for the band form")
        flux, image, shift_dev = self._begin_pass(flux, stride, shifts, norm, patch_norm)
        # (what every entry takes behind the image and in front of its outputs)
        value = (int(bool(marginalize)), c_float(value_scale), ptr(value_out), int(accumulate_value), c_float(grad_coef))
        outputs = (ptr(grad), ptr(argmax_out), shift_dev)
        if jitter is None and subpix is None:
            if band_out is None:
                check(_hip.lib().jd_gmm_prior_fwd_bwd(*image, int(patch_rows[0]), int(patch_rows[1]), *value, *outputs,
                                                      int(phases), stream_ptr(flux.device)))
                return
            if grad is not None or argmax_out is not None:
                raise ValueError("band_out excludes grad and argmax_out")
            return self._band_pass(flux, image, patch_rows, value, band_out)
        if band_out is not None or phases != 3 or tuple(patch_rows) != (0, -1) or (jitter is not None and subpix is not None):
            what = "a jittered patch grid" if jitter is not None else "a sub-pixel cycle spin"
            raise ValueError(f"{what} evaluates the whole prior: no patch_rows, band_out or phases, and no second variant")
        if jitter is not None:
            return self._jitter_pass(flux, image, jitter, value, outputs)
        return self._subpix_pass(flux, image, subpix, value, outputs)

    def _begin_pass(self, flux, stride, shifts, norm, patch_norm):
        """What every prior entry begins with: the norms of the call go to the handle, the flux is one HIP image, the roll is
        a host pair and, for `DeviceShifts`, a device address the kernels read instead.  Returns the contiguous flux, the
        leading arguments (handle, flux, H, W, stride, shift_y, shift_x) of the entries, and that address (or None)."""
        flux = require_hip_tensor(flux, "flux")
        self.set_image_norm(norm)
        self.set_patch_norm(patch_norm)
        H, W = flux.shape[-2:]
        if flux.numel() != H * W:
            raise ValueError("flux must be a single (H, W) image")
        shift_dev = None
        if isinstance(shifts, DeviceShifts):  # the kernels read the roll from device memory (captured graphs)
            shift_dev, shifts = ptr(shifts.dev), shifts.host
        sy, sx = (0, 0) if shifts is None else shifts
        return flux, (self._handle, ptr(flux), H, W, int(stride), int(sy), int(sx)), shift_dev

    def _band_pass(self, flux, image, patch_rows, value, band_out):
        H, W, stride = image[2:5]
        y0, y1 = band_rows(patch_rows, stride, H)
        if band_out.numel() < (y1 - y0) * W:
            raise ValueError(f"band_out holds {band_out.numel()} values, rows [{y0}, {y1}) x {W} need {(y1 - y0) * W}")
        check(_hip.lib().jd_gmm_prior_band_fwd_bwd(*image, int(patch_rows[0]), int(patch_rows[1]), *value, ptr(band_out),
                                                   stream_ptr(flux.device)))

    def _subpix_pass(self, flux, image, subpix, value, outputs):
        offset_dev = None
        if isinstance(subpix, DeviceShifts):
            offset_dev, subpix = ptr(subpix.dev), subpix.host
        x0, y0 = subpix
        check(_hip.lib().jd_gmm_prior_subpix_fwd_bwd(*image, c_float(x0), c_float(y0), *value, *outputs, offset_dev,
                                                     stream_ptr(flux.device)))

    def _jitter_pass(self, flux, image, jitter, value, outputs):
        H, W, stride = image[2:5]
        patch = 8 if self.D == 64 else 16
        if self._jitter_ring is None:
            self._jitter_ring = JitterRing(flux.device)
        ring = self._jitter_ring
        jitter_y, jitter_x, slot = ring.send(jitter, jitter_counts((H, W), patch, stride), patch - stride)
        check(_hip.lib().jd_gmm_prior_jitter_fwd_bwd(*image, ptr(jitter_y), ptr(jitter_x), *value, *outputs,
                                                     stream_ptr(flux.device)))
        if slot is not None:
            with torch.cuda.device(flux.device):
                ring.done(slot)

    def prior_image_table(self, patch_images):
        """The (K, P, P) table of `prior_image` on the handle's device, float32: uploaded once and kept while the caller
        keeps passing the same values (one table per handle: the eigen-images of the mixture, as a rule)."""
        patch = 8 if self.D == 64 else 16
        table = np.ascontiguousarray(patch_images, dtype=np.float32)
        if table.shape != (self.K, patch, patch):
            raise ValueError(f"patch_images must have shape ({self.K}, {patch}, {patch}), got {table.shape}")
        if self._prior_table is None or not np.array_equal(self._prior_table[0], table):
            self._prior_table = (table.copy(), torch.from_numpy(table).to(self.device))
        return self._prior_table[1]

    def prior_image(self, flux, stride, shifts, table, out, scale=1.0, accumulate=False, norm=None):
        """``out (+)= scale *`` the prior image of one draw (jd_gmm_prior_image): every patch of the rolled, normed flux
        replaced by ``table[arg-max component] + patch mean``, blended with the trapezoid pixel weights, un-rolled and sent
        through the inverse of ``norm``.  ``table``: (K, P, P) float32 on the flux's device (`prior_image_table`); ``out``:
        (H, W) float32 there.  Always the max mode and the subtract-mean patch norm; no host synchronisation."""
        flux, image, shift_dev = self._begin_pass(flux, stride, shifts, norm, None)
        if isinstance(out, torch.Tensor) and not out.is_contiguous():
            raise ValueError("out must be contiguous: the kernel writes it in place")
        table, out = require_hip_tensor(table, "table"), require_hip_tensor(out, "out")
        patch = 8 if self.D == 64 else 16
        if table.numel() != self.K * patch * patch or out.numel() != flux.numel():
            raise ValueError(f"table must hold {self.K} x {patch} x {patch} values and out the image's {flux.numel()}")
        check(_hip.lib().jd_gmm_prior_image(*image, ptr(table), c_float(scale), ptr(out), int(bool(accumulate)), shift_dev,
                                            stream_ptr(flux.device)))

    def prior_fwd_bwd_step(self, flux, stride, shifts, value_out, value_scale, grad_coef, step, marginalize=False,
                           accumulate_value=False, phases=3, norm=None, patch_norm=None):
        """The whole prior with the component's optimizer step in the epilogue of its gather kernel
        (jd_gmm_prior_fwd_bwd_step; ``step``: a filled `_hip.Step`).  Raises RuntimeError where the library does not
        support it (stride < 4): the caller then evaluates the prior and steps separately."""
        flux, image, shift_dev = self._begin_pass(flux, stride, shifts, norm, patch_norm)
        check(
            _hip.lib().jd_gmm_prior_fwd_bwd_step(
                *image, int(bool(marginalize)), c_float(value_scale), ptr(value_out), int(accumulate_value),
                c_float(grad_coef), ctypes.byref(step), shift_dev, int(phases), stream_ptr(flux.device),
            )
        )

    def screen_clock(self):
        """(MHz, samples): the shader clock inside the screen kernel since the last call (jd_gmm_screen_clock; the first call
        arms the handle and returns (0.0, 0); synchronises the device)."""
        mhz, samples = ctypes.c_double(0.0), c_int(0)
        check(_hip.lib().jd_gmm_screen_clock(self._handle, ctypes.byref(mhz), ctypes.byref(samples)))
        return float(mhz.value), int(samples.value)

    def screen_stats(self):
        """(generation, fell_back, bucket_slots, patches, rows_per_patch) of the last screened pass that has finished
        (jd_gmm_screen_stats; no synchronisation)."""
        out = (c_int * 5)()
        check(_hip.lib().jd_gmm_screen_stats(self._handle, out))
        return tuple(int(v) for v in out)

    def estimate_log_prob(self, x):
        x = require_hip_tensor(x, "x")
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError(f"x must have shape (n, {self.D}), got {tuple(x.shape)}")
        out = torch.empty((x.shape[0], self.K), dtype=torch.float32, device=x.device)
        if x.shape[0]:
            check(_hip.lib().jd_gmm_estimate_log_prob(self._handle, ptr(x), x.shape[0], ptr(out), stream_ptr(x.device)))
        return out


# ------------------------------------------------------------------------------------------
# autograd seams
# ------------------------------------------------------------------------------------------
class ConvSameFunction(torch.autograd.Function):
    """out = conv_same(image * scale, psf) through rocFFT; backward = correlation with the PSF.
    Stands where the reference calls `convolve_fft_torch` (jolideco/utils/torch.py:347-370)."""

    @staticmethod
    def forward(ctx, image, scale, khat, plan):
        ctx.plan, ctx.scale, ctx.khat = plan, scale, khat
        ctx.shape = image.shape
        return plan.conv_same(image, scale, khat).reshape(image.shape)

    @staticmethod
    def backward(ctx, grad_out):
        grad = ctx.plan.conv_same_adjoint(grad_out.contiguous(), ctx.scale, ctx.khat)
        return grad.reshape(ctx.shape), None, None, None


class PoissonNLLFunction(torch.autograd.Function):
    """nn.PoissonNLLLoss(log_input=False, reduction='mean', eps=1e-25, full=True) (loss.py:35-37)."""

    @staticmethod
    def forward(ctx, npred, counts, stirling):
        npred = require_hip_tensor(npred, "npred")
        counts = require_hip_tensor(counts, "counts")
        loss = torch.empty(1, dtype=torch.float32, device=npred.device)
        grad = torch.empty_like(npred)
        check(
            _hip.lib().jd_poisson_nll(
                ptr(npred), ptr(counts), npred.numel(), c_float(stirling), c_float(POISSON_EPS), ptr(loss), ptr(grad),
                stream_ptr(npred.device),
            )
        )
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return grad * grad_loss, None, None


class GMMPatchPriorFunction(torch.autograd.Function):
    """Scalar GMM patch log-prior with its HIP gradient (priors/patches/core.py:227-246)."""

    @staticmethod
    def forward(ctx, flux, handle, stride, shifts, marginalize, value_scale, norm=None, patch_norm=None, variant=None):
        """``variant``: None, or the keyword of `GmmHandle.prior_fwd_bwd` a staged pass is reached under and its draw:
        ("subpix", (x0, y0)) or ("jitter", (jitter_y, jitter_x))."""
        image = require_hip_tensor(flux, "flux")
        value = torch.empty(1, dtype=torch.float32, device=image.device)
        grad = None
        if flux.requires_grad:
            grad = torch.zeros(image.shape[-2:], dtype=torch.float32, device=image.device)
        handle.prior_fwd_bwd(
            image.reshape(image.shape[-2:]), stride, shifts, value, value_scale, grad=grad, grad_coef=value_scale,
            marginalize=marginalize, norm=norm, patch_norm=patch_norm, **({} if variant is None else dict([variant])),
        )
        ctx.grad, ctx.shape = grad, flux.shape
        return value.reshape(())

    @staticmethod
    def backward(ctx, grad_value):
        # (ctx.grad is the finished gradient with respect to the raw flux: the library applied the norm's chain rule)
        return (ctx.grad * grad_value).reshape(ctx.shape), None, None, None, None, None, None, None, None


def elementwise_prior_subpix(kind, flux, alpha, beta, log_const, shifts, value_out, grad_coef, grad=None):
    """InverseGammaPrior / ExponentialPrior with sub-pixel cycle spin (jd_elementwise_prior_subpix_fwd_bwd): the prior on
    the 3 x 3 stencil of ``shifts`` = (x0, y0) -- or a `DeviceShifts` whose ``dev`` holds them as two float32 in device
    memory (planned epochs).  value -> ``value_out``; ``grad += grad_coef * d sum(v) / d flux`` when ``grad`` is given."""
    flux = require_hip_tensor(flux, "flux")
    H, W = flux.shape[-2:]
    if flux.numel() != H * W:
        raise ValueError("flux must be a single (H, W) image")
    offset_dev = None
    if isinstance(shifts, DeviceShifts):
        offset_dev, shifts = ptr(shifts.dev), shifts.host
    x0, y0 = shifts
    check(
        _hip.lib().jd_elementwise_prior_subpix_fwd_bwd(
            int(kind), ptr(flux), int(H), int(W), c_float(alpha), c_float(beta), c_float(log_const), c_float(x0), c_float(y0),
            offset_dev, ptr(value_out), c_float(grad_coef), ptr(grad), stream_ptr(flux.device),
        )
    )


class ElementwisePriorFunction(torch.autograd.Function):
    """InverseGammaPrior / ExponentialPrior value and gradient (priors/core.py:207-226,308-326); ``shifts`` = (x0, y0):
    the sub-pixel cycle-spin form."""

    @staticmethod
    def forward(ctx, flux, kind, alpha, beta, log_const, shifts=None):
        image = require_hip_tensor(flux, "flux")
        value = torch.empty(1, dtype=torch.float32, device=image.device)
        grad = torch.zeros_like(image) if flux.requires_grad else None
        if shifts is not None:
            elementwise_prior_subpix(kind, image, alpha, beta, log_const, shifts, value, 1.0 / image.numel(), grad)
        else:
            check(
                _hip.lib().jd_elementwise_prior_fwd_bwd(
                    int(kind), ptr(image), image.numel(), c_float(alpha), c_float(beta), c_float(log_const), ptr(value),
                    c_float(1.0 / image.numel()), ptr(grad), stream_ptr(image.device),
                )
            )
        ctx.grad, ctx.shape = grad, flux.shape
        return value.reshape(())

    @staticmethod
    def backward(ctx, grad_value):
        return (ctx.grad * grad_value).reshape(ctx.shape), None, None, None, None, None


def smoothness_prior(plan, khat, flux, value_out, grad_coef=0.0, grad=None):
    """SmoothnessPrior (jd_smoothness_prior_fwd_bwd): value_out <- -sum(flux * (K (*) flux)),
    ``grad += grad_coef * (-2 K (*) flux)`` when ``grad`` is given; ``khat``: the kernel's operator for ``plan``."""
    flux = plan._check_image(flux, "flux")
    check(
        _hip.lib().jd_smoothness_prior_fwd_bwd(
            plan._handle, ptr(khat), ptr(flux), ptr(value_out), c_float(grad_coef), ptr(grad), stream_ptr(flux.device),
        )
    )


class SmoothnessPriorFunction(torch.autograd.Function):
    """SmoothnessPrior value with its HIP gradient (priors/core.py:382-384)."""

    @staticmethod
    def forward(ctx, flux, plan, khat):
        image = require_hip_tensor(flux, "flux")
        value = torch.empty(1, dtype=torch.float32, device=image.device)
        grad = torch.zeros_like(image) if flux.requires_grad else None
        smoothness_prior(plan, khat, image, value, 1.0, grad)
        ctx.grad, ctx.shape = grad, flux.shape
        return value.reshape(())

    @staticmethod
    def backward(ctx, grad_value):
        return (ctx.grad * grad_value).reshape(ctx.shape), None, None


def _sparse_vectors(param, x_pos, y_pos):
    param = require_hip_tensor(param, "flux parameter")
    n = param.numel()
    for name, t in (("x_pos", x_pos), ("y_pos", y_pos)):
        require_hip_tensor(t, name)
        if t.numel() != n:
            raise ValueError(f"{name} holds {t.numel()} values for {n} sources")
    limit = _hip.lib().jd_sparse_max_sources()
    if not 1 <= n <= limit:
        raise ValueError(f"a sparse flux component holds 1 to {limit} sources, got {n}")
    return n


def sparse_render(param, x_pos, y_pos, use_log_flux, out):
    """out (H, W) <- the image of the point sources (jd_sparse_render): sum_n wx_n wy_n f_n with the bilinear weights of
    the reference's `grid_weights`, f = exp(param) for ``use_log_flux``; every pixel is written."""
    n = _sparse_vectors(param, x_pos, y_pos)
    out = require_hip_tensor(out, "out")
    H, W = out.shape[-2:]
    if out.numel() != H * W:
        raise ValueError("out must be a single (H, W) image")
    check(_hip.lib().jd_sparse_render(ptr(param), ptr(x_pos), ptr(y_pos), n, int(bool(use_log_flux)), int(H), int(W), ptr(out),
                                      stream_ptr(out.device)))
    return out


def sparse_backward(param, x_pos, y_pos, use_log_flux, grad_image, grad_param, grad_x, grad_y):
    """(grad_param, grad_x, grad_y) <- the gradients of the three vectors given ``grad_image`` = d loss / d image
    (jd_sparse_backward); assigned, not accumulated."""
    n = _sparse_vectors(param, x_pos, y_pos)
    grad_image = require_hip_tensor(grad_image, "grad_image")
    H, W = grad_image.shape[-2:]
    if grad_image.numel() != H * W:
        raise ValueError("grad_image must be a single (H, W) image")
    for t in (grad_param, grad_x, grad_y):
        if require_hip_tensor(t, "gradient vector").numel() != n:
            raise ValueError("gradient vectors must hold one value per source")
    check(_hip.lib().jd_sparse_backward(ptr(param), ptr(x_pos), ptr(y_pos), n, int(bool(use_log_flux)), int(H), int(W),
                                        ptr(grad_image), ptr(grad_param), ptr(grad_x), ptr(grad_y),
                                        stream_ptr(grad_image.device)))


class SparseRenderFunction(torch.autograd.Function):
    """(1, 1, H, W) image of a sparse flux component, differentiable with respect to its flux parameter and positions
    (models/core.py:216-232)."""

    @staticmethod
    def forward(ctx, param, x_pos, y_pos, shape, use_log_flux):
        H, W = (int(v) for v in shape)
        image = torch.empty((1, 1, H, W), dtype=torch.float32, device=param.device)
        vectors = [v.detach().contiguous() for v in (param, x_pos, y_pos)]
        sparse_render(*vectors, use_log_flux, image)
        ctx.save_for_backward(*vectors)
        ctx.use_log_flux = use_log_flux
        return image

    @staticmethod
    def backward(ctx, grad_image):
        param, x_pos, y_pos = ctx.saved_tensors
        grads = [torch.empty_like(param) for _ in range(3)]
        sparse_backward(param, x_pos, y_pos, ctx.use_log_flux, grad_image.contiguous(), *grads)
        return grads[0], grads[1], grads[2], None, None


MULTISCALE_MAX_LEVELS = 5  # JD_MULTISCALE_MAX_LEVELS of include/jolideco_hip.h
MULTISCALE_FACTORS = (1, 2, 4, 8, 16)


def _host_floats(values):
    """(ctypes float array, length) of a short host vector (the taps of a level, the level coefficients)."""
    values = [float(v) for v in values]
    return (c_float * len(values))(*values), len(values)


def multiscale_down(src, f, taps, d_out, g_out=None, dd_zero=None, shifts=None):
    """One level of the multi-scale pyramid (jd_multiscale_down): ``g_out`` <- K (*) ``src`` (K = outer(taps, taps), "same",
    zero padded; None: not stored), ``d_out`` <- its ``f`` x ``f`` means (floor), ``dd_zero`` <- 0.  ``shifts``: the loads
    read ``src`` rolled by this pair (rows, columns), as `torch.roll` would."""
    src = require_hip_tensor(src, "src")
    H, W = src.shape[-2:]
    sy, sx = (0, 0) if shifts is None else (int(shifts[0]) % H, int(shifts[1]) % W)
    if tuple(d_out.shape[-2:]) != (H // f, W // f):
        raise ValueError(f"d_out must have shape {(H // f, W // f)}, got {tuple(d_out.shape[-2:])}")
    arr, n = _host_floats(taps)
    check(_hip.lib().jd_multiscale_down(ptr(src), H, W, int(f), arr, n, sy, sx, ptr(g_out), ptr(d_out), ptr(dd_zero),
                                        stream_ptr(src.device)))


def multiscale_up_adjoint(dd, f, taps, out, dg=None, shifts=None, rolled=False, value=None):
    """Adjoint of one level (jd_multiscale_up_adjoint): ``out`` <- K^T (*) (``dg`` + replicate_f(``dd``) / f^2); with
    ``rolled`` the result is ADDED to ``out`` at the un-rolled pixel (the session's gradient image).  ``value``:
    (level values on the device, host coefficients, value_out) -- the launch also writes their weighted sum."""
    dd = require_hip_tensor(dd, "dd")
    H, W = out.shape[-2:]
    sy, sx = (0, 0) if shifts is None else (int(shifts[0]) % H, int(shifts[1]) % W)
    if tuple(dd.shape[-2:]) != (H // f, W // f):
        raise ValueError(f"dd must have shape {(H // f, W // f)}, got {tuple(dd.shape[-2:])}")
    arr, n = _host_floats(taps)
    vals, coefs, n_values, value_out = None, None, 0, None
    if value is not None:
        vals, (coefs, n_values), value_out = ptr(value[0]), _host_floats(value[1]), ptr(value[2])
    check(_hip.lib().jd_multiscale_up_adjoint(ptr(dg), ptr(dd), H, W, int(f), arr, n, ptr(out), int(bool(rolled)), sy, sx,
                                              vals, coefs, n_values, value_out, stream_ptr(out.device)))


def multiscale_value(values, coefs, value_out):
    """value_out <- sum_i coefs[i] * values[i] on the device (jd_multiscale_value: a forward-only multi-scale call)."""
    arr, n = _host_floats(coefs)
    check(_hip.lib().jd_multiscale_value(ptr(values), arr, n, ptr(value_out), stream_ptr(value_out.device)))


class MultiScalePriorFunction(torch.autograd.Function):
    """Scalar multi-scale log-prior with its HIP gradient (priors/patches/core.py:288-326): the prior's own device pass with
    coefficient 1 into a fresh gradient image."""

    @staticmethod
    def forward(ctx, flux, prior, shifts):
        image = require_hip_tensor(flux, "flux")
        value = torch.empty(1, dtype=torch.float32, device=image.device)
        grad = torch.zeros(image.shape[-2:], dtype=torch.float32, device=image.device) if flux.requires_grad else None
        prior.device_fwd_bwd(image, value, grad=grad, coef=1.0, shifts=shifts)
        ctx.grad, ctx.shape = grad, flux.shape
        return value.reshape(())

    @staticmethod
    def backward(ctx, grad_value):
        return (ctx.grad * grad_value).reshape(ctx.shape), None, None


def band_rows(patch_rows, stride, H, patch=8):
    """Pixel rows [y_begin, y_end) of the rolled frame that the patch rows ``patch_rows = (begin, end)`` cover
    (``end < 0``: up to the last patch row); an empty shard covers no row."""
    n_py = (H - patch) // stride + 1
    begin, end = patch_rows
    end = n_py if end < 0 else end
    if end <= begin:
        return begin * stride, begin * stride
    return begin * stride, (end - 1) * stride + patch


def add_rolled_bands(grad, shifts, bands, chunk, y_ranges):
    """grad (un-rolled image) += the bands of the rolled frame (jd_add_rolled_bands): ``bands`` is the flat device buffer
    of an all-gather, band b starts at ``b * chunk`` and holds the rows ``y_ranges[b] = (y_begin, y_end)``."""
    grad = require_hip_tensor(grad, "grad")
    bands = require_hip_tensor(bands, "bands")
    H, W = grad.shape[-2:]
    n = len(y_ranges)
    if bands.numel() < (n - 1) * chunk + max((y1 - y0) * W for y0, y1 in y_ranges):
        raise ValueError("bands buffer too small for n_bands pieces of `chunk` values")
    sy, sx = (0, 0) if shifts is None else shifts
    y0 = (c_int * n)(*[int(r[0]) for r in y_ranges])
    y1 = (c_int * n)(*[int(r[1]) for r in y_ranges])
    check(_hip.lib().jd_add_rolled_bands(ptr(grad), H, W, int(sy), int(sx), ptr(bands), int(chunk), n, y0, y1, stream_ptr(grad.device)))


def add_rolled_bands_step(shape, shifts, bands, chunk, y_ranges, step):
    """The sum of `add_rolled_bands` followed at once by the optimizer step of the image (jd_add_rolled_bands_step):
    ``step`` is the `_hip.Step` of the component, whose gradient image is only read.  Needs W % 4 == 0."""
    bands = require_hip_tensor(bands, "bands")
    H, W = (int(v) for v in shape[-2:])
    n = len(y_ranges)
    if bands.numel() < (n - 1) * chunk + max((y1 - y0) * W for y0, y1 in y_ranges):
        raise ValueError("bands buffer too small for n_bands pieces of `chunk` values")
    sy, sx = (0, 0) if shifts is None else shifts
    y0 = (c_int * n)(*[int(r[0]) for r in y_ranges])
    y1 = (c_int * n)(*[int(r[1]) for r in y_ranges])
    check(_hip.lib().jd_add_rolled_bands_step(H, W, int(sy), int(sx), ptr(bands), int(chunk), n, y0, y1, ctypes.byref(step),
                                              stream_ptr(bands.device)))


def sum_images(out, srcs):
    """out <- ((srcs[0] + srcs[1]) + ...) (jd_sum_images: the summed flux of components that share one forward operator)."""
    out = require_hip_tensor(out, "out")
    if not 1 <= len(srcs) <= 4:
        raise ValueError("1 to 4 source images")
    for t in srcs:
        require_hip_tensor(t, "source")
        if t.numel() != out.numel() or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("sources must be contiguous float32 images of the size of `out`")
    check(_hip.lib().jd_sum_images(ptr(out), ptr_array(list(srcs)), len(srcs), out.numel(), stream_ptr(out.device)))
    return out


def copy_image_to(src, dsts):
    """dsts[d] <- src for every d (jd_copy_image_to: one gradient image for all components that share an operator)."""
    src = require_hip_tensor(src, "src")
    if not 1 <= len(dsts) <= 4:
        raise ValueError("1 to 4 destination images")
    for t in dsts:
        require_hip_tensor(t, "destination")
        if t.numel() != src.numel() or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("destinations must be contiguous float32 images of the size of `src`")
    check(_hip.lib().jd_copy_image_to(ptr(src), ptr_array(list(dsts)), len(dsts), src.numel(), stream_ptr(src.device)))


def adam_bias_terms(step, lr, beta1, beta2):
    """step_size and sqrt(bias_correction2) exactly as torch.optim.Adam computes them
    (python floats = float64), torch/optim/adam.py `_single_tensor_adam`."""
    bias1 = 1 - beta1**step
    bias2 = 1 - beta2**step
    return lr / bias1, math.sqrt(bias2)


class GmmFitHandle:
    """Work space of the EM step kernel (jd_gmm_fit, csrc/gmm_fit.hip) for mixtures of ``n_components`` components over
    ``n_features`` = 64 or 256 features on one device.  ``max_blocks`` bounds the sets of partial sums (0: the default)."""

    def __init__(self, n_features, n_components, device, max_blocks=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GmmFitHandle needs a HIP device (no CPU fallback)")
        self.D, self.K = int(n_features), int(n_components)
        handle = c_void_p()
        with torch.cuda.device(self.device):
            check(_hip.lib().jd_gmm_fit_create(self.D, self.K, int(max_blocks), ctypes.byref(handle)))
        self._handle = handle
        size = self.K * (1 + self.D + self.D * self.D) + 1
        self.sums = torch.empty(size, dtype=torch.float64, device=self.device)
        self._host = torch.empty(size, dtype=torch.float64).pin_memory()

    def close(self):
        if self._handle is not None:
            _hip.lib().jd_gmm_fit_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, x, means, precisions_cholesky, const_k):
        """The sums of one E-step over the patches ``x`` (n, D) for float32 device parameters: float64 numpy arrays
        ``(sum r (K,), sum r d (K, D), sum r d d^T (K, D, D), sum lse)`` with d = x - means[k]; synchronises on the copy."""
        K, D = self.K, self.D
        x = require_hip_tensor(x, "patches")
        if x.ndim != 2 or x.shape[1] != D or not x.is_contiguous():
            raise ValueError(f"patches must be a contiguous (n, {D}) tensor, got {tuple(x.shape)}")
        for t, shape, name in ((means, (K, D), "means"), (precisions_cholesky, (K, D, D), "precisions_cholesky"), (const_k, (K,), "const_k")):
            require_hip_tensor(t, name)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
        with torch.cuda.device(self.device):
            check(_hip.lib().jd_gmm_fit_step(self._handle, ptr(x), x.shape[0], ptr(means), ptr(precisions_cholesky), ptr(const_k),
                                             c_void_p(self.sums.data_ptr()), stream_ptr(self.device)))
            self._host.copy_(self.sums, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        flat = self._host.numpy()
        s0 = flat[:K].copy()
        s1 = flat[K:K + K * D].reshape(K, D).copy()
        s2 = flat[K + K * D:K + K * D + K * D * D].reshape(K, D, D).copy()
        return s0, s1, s2, float(flat[-1])

    def step_labels(self, x, means, labels):
        """The same sums for hard assignments r_nk = [labels[n] == k] (jd_gmm_fit_step_labels): ``labels`` is an int32
        device tensor (n,); a label outside [0, K) contributes nothing.  Returns ``(sum r, sum r d, sum r d d^T)``."""
        K, D = self.K, self.D
        x = require_hip_tensor(x, "patches")
        if x.ndim != 2 or x.shape[1] != D or not x.is_contiguous():
            raise ValueError(f"patches must be a contiguous (n, {D}) tensor, got {tuple(x.shape)}")
        require_hip_tensor(means, "means")
        if tuple(means.shape) != (K, D) or not means.is_contiguous():
            raise ValueError(f"means must be a contiguous {(K, D)} tensor, got {tuple(means.shape)}")
        labels = _require_labels(labels, x.shape[0])
        with torch.cuda.device(self.device):
            check(_hip.lib().jd_gmm_fit_step_labels(self._handle, ptr(x), x.shape[0], ptr(means), c_void_p(labels.data_ptr()),
                                                    c_void_p(self.sums.data_ptr()), stream_ptr(self.device)))
            self._host.copy_(self.sums, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        flat = self._host.numpy()
        s0 = flat[:K].copy()
        s1 = flat[K:K + K * D].reshape(K, D).copy()
        s2 = flat[K + K * D:K + K * D + K * D * D].reshape(K, D, D).copy()
        return s0, s1, s2


def _require_labels(labels, n):
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
        raise RuntimeError("labels must be a HIP tensor (no CPU fallback)")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
        raise ValueError(f"labels must be a contiguous int32 ({n},) tensor, got {labels.dtype} {tuple(labels.shape)}")
    return labels


class KMeansHandle:
    """Work space of the Lloyd step (jd_kmeans, csrc/kmeans.hip) for ``n_clusters`` centres over ``n_features`` = 64 or 256
    features on one device.  ``max_blocks`` bounds the sets of partial sums (0: the default)."""

    def __init__(self, n_features, n_clusters, device, max_blocks=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("KMeansHandle needs a HIP device (no CPU fallback)")
        self.D, self.K = int(n_features), int(n_clusters)
        handle = c_void_p()
        with torch.cuda.device(self.device):
            check(_hip.lib().jd_kmeans_create(self.D, self.K, int(max_blocks), ctypes.byref(handle)))
        self._handle = handle
        size = self.K * (1 + self.D) + 3
        self.sums = torch.empty(size, dtype=torch.float64, device=self.device)
        self._host = torch.empty(size, dtype=torch.float64).pin_memory()

    def close(self):
        if self._handle is not None:
            _hip.lib().jd_kmeans_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def launch(self, x, centres, labels):
        """One Lloyd step on the current stream, without a copy or a synchronisation: ``labels`` is rewritten and
        ``self.sums`` holds [count | sum x | inertia | changed | unassigned] once the stream has run."""
        K, D = self.K, self.D
        x = require_hip_tensor(x, "patches")
        if x.ndim != 2 or x.shape[1] != D or not x.is_contiguous():
            raise ValueError(f"patches must be a contiguous (n, {D}) tensor, got {tuple(x.shape)}")
        require_hip_tensor(centres, "centres")
        if tuple(centres.shape) != (K, D) or not centres.is_contiguous():
            raise ValueError(f"centres must be a contiguous {(K, D)} tensor, got {tuple(centres.shape)}")
        labels = _require_labels(labels, x.shape[0])
        with torch.cuda.device(self.device):
            check(_hip.lib().jd_kmeans_step(self._handle, ptr(x), x.shape[0], ptr(centres), c_void_p(labels.data_ptr()),
                                            c_void_p(self.sums.data_ptr()), stream_ptr(self.device)))

    def step(self, x, centres, labels):
        """One Lloyd step over the patches ``x`` (n, D) for float32 device ``centres`` (K, D): ``labels`` (int32 device
        tensor (n,)) is read -- for the count of changes -- and rewritten; returns float64 numpy ``(count (K,), sum x (K, D),
        inertia, changed, unassigned)``; synchronises on the copy."""
        K, D = self.K, self.D
        self.launch(x, centres, labels)
        with torch.cuda.device(self.device):
            self._host.copy_(self.sums, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        flat = self._host.numpy()
        return flat[:K].copy(), flat[K:K + K * D].reshape(K, D).copy(), float(flat[-3]), int(flat[-2]), int(flat[-1])

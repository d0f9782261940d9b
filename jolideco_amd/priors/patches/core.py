"""GMM patch prior (reference: jolideco/priors/patches/core.py:30-246)."""
import logging

import numpy as np
import torch

from ...utils.norms import IdentityImageNorm, ImageNorm, PatchNorm, SubtractMeanPatchNorm
from ...utils.numpy import gaussian_kernel_2d
from ...utils.torch import (
    TORCH_DEFAULT_DEVICE, cycle_spin_shifts, cycle_spin_shifts_many, get_default_generator, jitter_draws, jitter_grid,
    jitter_stride_check, subpixel_offsets,
)
from ..core import Prior
from .gmm import GaussianMixtureModel

__all__ = ["GMMPatchPrior", "SubpixelGMMPatchPrior", "JitteredGMMPatchPrior", "MultiScalePrior"]

log = logging.getLogger(__name__)


class GMMPatchPrior(Prior):
    """Patch prior: expected (max or marginal) GMM log-likelihood of all overlapping patches.

    Same constructor as the reference.  8x8 and 16x16 patches (64 / 256 features) have kernels; a 16x16 prior runs the
    whole-image dense pass only (`shardable`, `supports_fused_step`, `supports_phases` are False for it).  The two switches of
    this constructor that are not on its accelerated path (``cycle_spin_subpix``, ``jitter``) raise NotImplementedError
    instead of silently running something else; the sub-pixel cycle spin is the subclass `SubpixelGMMPatchPrior`, the
    jittered patch grid the subclass `JitteredGMMPatchPrior`.

    ``patch_norm``: `SubtractMeanPatchNorm` or `StandardizedSubtractMeanPatchNorm` (relative contrast, (p - mean) / mean),
    by default the one the mixture was trained with (``gmm.meta.patch_norm``, the ``PNPTYPE`` keyword of a table file).
    Both are fused into the kernels.  The standardized norm always takes the dense fp32 kernels -- the fp16 screen of the
    8x8 path is derived for mean-free patches and is not used for it -- and has no ``compute_error`` (`hessian_ones`).

    ``norm``: identity, asinh, fixed-max, sigmoid, atan, log or power image norm (`utils.norms`), applied on the device in
    front of the patch extraction; the gradient is the one with respect to the raw flux.  The norm's parameters are
    constants of the prior (the reference trains them unless ``frozen``): they go to the kernels by value with every
    call, and a captured epoch bakes them in.
    """

    def __init__(
        self,
        gmm=None,
        stride=None,
        cycle_spin=True,
        cycle_spin_subpix=False,
        generator=None,
        norm=None,
        patch_norm=None,
        jitter=False,
        marginalize=False,
        device=TORCH_DEFAULT_DEVICE,
    ):
        super().__init__()
        if gmm is None:
            gmm = GaussianMixtureModel.from_registry(name="zoran-weiss")
        self.gmm = gmm
        self.stride = gmm.meta.stride if stride is None else stride
        if self.stride is None:
            raise ValueError("stride must be given either explicitly or through gmm.meta.stride")
        self.cycle_spin = cycle_spin
        if cycle_spin_subpix:
            raise NotImplementedError("cycle_spin_subpix is not an option of GMMPatchPrior in jolideco_amd: the sub-pixel "
                                      "cycle spin is the class SubpixelGMMPatchPrior (same arguments)")
        if jitter:
            raise NotImplementedError(f"jitter is not an option of {type(self).__name__} in jolideco_amd: the jittered patch "
                                      "grid is the class JitteredGMMPatchPrior (same arguments)")
        self.cycle_spin_subpix = False  # (True in `SubpixelGMMPatchPrior` only)
        self.jitter = False  # (True in `JitteredGMMPatchPrior` only)
        # shifts are ALWAYS drawn from a host generator (torch default seed), see utils/torch.py
        self.generator = generator if generator is not None else get_default_generator("cpu")
        if self.generator.device.type != "cpu":
            raise ValueError("the cycle-spin generator must be a CPU generator")
        norm = norm if norm is not None else IdentityImageNorm()
        if not isinstance(norm, ImageNorm) or norm.device_kind is None:
            raise NotImplementedError(f"image norm {type(norm).__name__} is not implemented in jolideco_amd")
        self.norm = norm
        patch_norm = patch_norm if patch_norm is not None else gmm.meta.patch_norm
        if not isinstance(patch_norm, PatchNorm) or patch_norm.device_kind is None:
            raise NotImplementedError(f"patch norm {type(patch_norm).__name__} is not implemented in jolideco_amd")
        self.patch_norm = patch_norm
        self.marginalize = marginalize
        self.device = torch.device(device)
        self.last_shifts = None

    @property
    def patch_shape(self):
        return self.gmm.patch_shape

    # What a subclass with a staged pass (a variant) sets, beside `_draw_variant` and `_order_variant`:
    shift_kind = "roll"  # what `draw_shifts` returns: a pair of integer rolls or None; a variant: (that, the variant's draw)
    _variant_keyword = None  # the keyword of `GmmHandle.prior_fwd_bwd` the variant's draw goes under; such a prior is whole-image only
    _variant_form = None  # how the variant's draw is written in messages
    _no_hessian_ones = None  # why the variant has no `hessian_ones` (None: it has)

    @property
    def _full_path(self):
        """8x8 patches run every form of the pass; 16x16 patches (D = 256) and a variant have the whole-image pass only."""
        return tuple(self.patch_shape) == (8, 8) and self._variant_keyword is None

    @property
    def shardable(self):
        """The patch rows can be split over the ranks of a sharded joint fit (band output).  A prior that cannot is
        evaluated whole on rank 0, like the element-wise priors (`FitSession`)."""
        return self._full_path

    @property
    def supports_fused_step(self):
        """The optimizer step of the component can ride in the epilogue of this prior's last kernel (`device_fwd_bwd_step`)."""
        return self._full_path

    @property
    def supports_phases(self):
        """The pass splits into phase 1 (value + gradient rows: reads the flux only) and phase 2 (gather [+ step]): phase 1
        may run on a second stream beside the likelihood launches (`phases` of device_fwd_bwd[_step]; FitSession)."""
        return self._full_path

    @property
    def overlap(self):
        return max(self.patch_shape) - self.stride

    @property
    def log_like_weight(self):
        """stride^2 / patch area (priors/patches/core.py:222-225)."""
        return self.stride**2 / (self.patch_shape[0] * self.patch_shape[1])

    def _draw_grid(self, shape):
        """What the variant's draw needs to know of an image of ``shape``; a shape the variant cannot take raises here"""
        return None

    def draw_shifts(self, shape=None):
        """One draw: the pair of cycle-spin rolls (None when cycle_spin is off); a variant returns the pair (that, its own
        draw) -- the roll is drawn first, the reference's order.  ``shape``: the image's, for a variant whose draw depends
        on it."""
        grid = self._draw_grid(shape)  # (a refused shape raises before the generator advances)
        shifts = cycle_spin_shifts(self.patch_shape, self.generator) if self.cycle_spin else None
        if self._variant_keyword is not None:
            shifts = (shifts, self._draw_variant(grid))
        self.last_shifts = shifts
        return shifts

    def draw_shifts_many(self, n, shape=None):
        """The next `n` draws, in order (an epoch's worth, `FitSession._plan_epoch`)."""
        if self._variant_keyword is not None:  # (the roll's and the variant's draws alternate per evaluation: one by one)
            return [self.draw_shifts(shape) for _ in range(n)]
        if not self.cycle_spin:
            self.last_shifts = None
            return [None] * n
        shifts = cycle_spin_shifts_many(self.patch_shape, self.generator, n)
        self.last_shifts = shifts[-1]
        return shifts

    def __call__(self, flux, mask=None):
        """Differentiable log-prior of a (1, 1, H, W) HIP tensor; draws once, for the flux's shape."""
        from ...ops import GMMPatchPriorFunction

        roll, variant = self._split_shifts(self.draw_shifts(flux.shape))
        scale = self.log_like_weight / flux.numel()
        return GMMPatchPriorFunction.apply(
            flux, self.gmm.handle(flux.device), self.stride, roll, self.marginalize, scale, self.norm, self.patch_norm,
            None if variant is None else (self._variant_keyword, variant),
        )

    def _split_shifts(self, shifts):
        """(roll, the variant's draw as the handle takes it -- or None) of a draw of `draw_shifts`."""
        if self._variant_keyword is None:
            return shifts, None
        variant = self._order_variant(shifts[1]) if isinstance(shifts, tuple) and len(shifts) == 2 else None
        if variant is None:
            raise ValueError(f"a {type(self).__name__} takes the pair (roll or None, {self._variant_form}) as shifts, got {shifts!r}")
        return shifts[0], variant

    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, patch_rows=None, shifts="draw", band_out=None, phases=3):
        """Fused path: value -> device scalar, ``grad += coef * d logprior / d flux``; with ``band_out`` the gradient of
        the shard ``patch_rows`` goes, un-accumulated, to the band of the rolled frame it covers (sharded joint fit).
        ``shifts``: a draw of `draw_shifts` ("draw": one for the flux's shape).  A variant runs the whole prior only."""
        if isinstance(shifts, str):
            shifts = self.draw_shifts(flux.shape)
        roll, variant = self._split_shifts(shifts)
        scale = self.log_like_weight / flux.numel()
        self.gmm.handle(flux.device).prior_fwd_bwd(
            flux.reshape(flux.shape[-2:]), self.stride, roll, value_out, scale, grad=grad, grad_coef=coef * scale,
            marginalize=self.marginalize, patch_rows=patch_rows or (0, -1), band_out=band_out, phases=phases, norm=self.norm,
            patch_norm=self.patch_norm, **({} if variant is None else {self._variant_keyword: variant}),
        )

    def device_fwd_bwd_step(self, flux, value_out, coef, step, shifts="draw", phases=3):
        """`device_fwd_bwd` of the WHOLE prior with the component's optimizer step applied by its gather kernel:
        ``step.grad_flux`` holds every other gradient term; theta, the moments and the new flux are written in place
        (jd_gmm_prior_fwd_bwd_step).  Same numbers as `device_fwd_bwd` followed by the stand-alone step."""
        if self._variant_keyword is not None:
            raise NotImplementedError(f"a {type(self).__name__} has no fused optimizer step: call device_fwd_bwd and step "
                                      "separately")
        if isinstance(shifts, str):
            shifts = self.draw_shifts()
        scale = self.log_like_weight / flux.numel()
        self.gmm.handle(flux.device).prior_fwd_bwd_step(
            flux.reshape(flux.shape[-2:]), self.stride, shifts, value_out, scale, coef * scale, step,
            marginalize=self.marginalize, phases=phases, norm=self.norm, patch_norm=self.patch_norm,
        )

    def _prior_image_inputs(self, flux, patch_images):
        """(flux as one HIP image, the table as the handle keeps it) of `prior_image`; every refusal is raised here, before
        the generator advances."""
        if self.jitter:
            raise ValueError("Computing prior images with jittering is not supported.")
        if self.cycle_spin_subpix:
            raise NotImplementedError("prior images with cycle_spin_subpix are not implemented: the reference leaves the "
                                      "sub-pixel un-shift open")
        if not isinstance(self.patch_norm, SubtractMeanPatchNorm):
            name = self.patch_norm.to_dict().get("type", type(self.patch_norm).__name__)
            raise NotImplementedError(f"prior images are not implemented for patch norm {name!r}: the formula adds back "
                                      "the patch mean only")
        patch = max(self.patch_shape)
        if not 1 <= self.stride < patch:
            raise ValueError(f"a prior image needs overlapping patches: stride {self.stride} is not in [1, {patch - 1}] "
                             "(the pixel weights' slope is 1 / overlap)")
        table = self.gmm.eigen_images if patch_images is None else np.asarray(patch_images)
        if table.shape != (self.gmm.n_components,) + tuple(self.patch_shape):
            raise ValueError(f"patch_images must have shape {(self.gmm.n_components,) + tuple(self.patch_shape)}, got {table.shape}")
        if isinstance(flux, torch.Tensor):
            if not flux.is_cuda:
                raise RuntimeError("flux must be a HIP tensor or a numpy array: jolideco_amd has no CPU path")
            image = flux.detach().to(torch.float32)
        else:
            image = torch.from_numpy(np.ascontiguousarray(flux, dtype=np.float32)).to(self.device)
        if image.ndim < 2 or image.numel() != image.shape[-2] * image.shape[-1]:
            raise ValueError(f"flux must be one image, (H, W) or (1, 1, H, W), got shape {tuple(image.shape)}")
        image = image.reshape(image.shape[-2:]).contiguous()
        if image.shape[0] < patch or image.shape[1] < patch:
            raise ValueError(f"flux {tuple(image.shape)} is smaller than a patch")
        return image, self.gmm.handle(image.device).prior_image_table(table)

    def prior_image(self, flux, patch_images=None):
        """What the prior believes ``flux`` looks like, for one draw of the cycle spin (reference:
        priors/patches/core.py:123-151, which cannot run as written; this is the formula its lines state): every patch of
        the rolled, normed flux is replaced by the table entry of its best-fitting component plus the patch mean -- the
        arg-max, also for a prior with ``marginalize=True`` --, the patches are blended with the trapezoid pixel weights, the
        roll is undone and the image goes through the norm's inverse.  On the device (jd_gmm_prior_image).

        flux : HIP tensor (1, 1, H, W) or (H, W), or numpy (H, W) (uploaded to ``prior.device``).
        patch_images : optional (K, P, P) array used instead of ``gmm.eigen_images`` -- the component means, samples, ...;
            unlike the eigen-images such a table does not depend on LAPACK's eigenvector signs.

        One `draw_shifts`: the generator advances as for one evaluation.  Returns a float32 numpy (H, W).  Raises for a
        jittered prior (ValueError, the reference's own refusal), a sub-pixel cycle spin or the standardized patch norm
        (NotImplementedError), ``stride == P`` or a table of the wrong shape (ValueError), before anything is drawn."""
        return self.prior_image_average(flux, n_average=1, patch_images=patch_images)

    def prior_image_average(self, flux, n_average=100, patch_images=None):
        """The mean of `prior_image` over ``n_average`` draws of the cycle spin (priors/patches/core.py:153-175): accumulated
        on the device with a fixed order of additions, one copy to the host at the end."""
        n_average = int(n_average)
        if n_average < 1:
            raise ValueError(f"n_average must be at least 1, got {n_average}")
        image, table = self._prior_image_inputs(flux, patch_images)
        handle = self.gmm.handle(image.device)
        out = torch.empty_like(image)
        for draw in range(n_average):
            handle.prior_image(image, self.stride, self.draw_shifts(image.shape), table, out, scale=1.0 / n_average,
                               accumulate=draw > 0, norm=self.norm)
        return out.cpu().numpy()

    def hessian_ones(self, flux):
        """Every patch has its mean subtracted before the mixture sees it, so a constant vector is in the null
        space of each patch's quadratic form: Hessian x ones is exactly zero (the reference's double backward
        returns rounding noise there).  One pair of shifts is drawn, as the reference's evaluation does.
        The argument holds for `SubtractMeanPatchNorm` only: under the standardized norm a constant added to a patch
        changes x = (p - m) / m, and there is no kernel for that Hessian product."""
        self.check_hessian_ones()
        self.draw_shifts(flux.shape)
        return torch.zeros_like(flux)

    def check_hessian_ones(self):
        """Raise where `hessian_ones` (``compute_error=True``) is not available: any patch norm but subtract-mean, and a
        variant that says so (`_no_hessian_ones`)."""
        if self._no_hessian_ones:
            raise NotImplementedError(f"compute_error=True is not implemented for a GMMPatchPrior with {self._no_hessian_ones}")
        if not isinstance(self.patch_norm, SubtractMeanPatchNorm):
            name = self.patch_norm.to_dict().get("type", type(self.patch_norm).__name__)
            raise NotImplementedError(
                f"compute_error=True is not implemented for a GMMPatchPrior with patch norm {name!r}: the Hessian "
                "product with ones is zero for 'subtract-mean' only"
            )

    def n_patch_rows(self, shape):
        return (shape[-2] - self.patch_shape[0]) // self.stride + 1

    def to_dict(self):
        data = super().to_dict()
        data.update(
            stride=int(self.stride), cycle_spin=bool(self.cycle_spin), cycle_spin_subpix=bool(self.cycle_spin_subpix),
            jitter=bool(self.jitter),
            gmm=self.gmm.to_dict(), norm=self.norm.to_dict(), patch_norm=self.patch_norm.to_dict(),
            device=str(self.device),
        )
        if self.marginalize:
            data["marginalize"] = True
        return data

    @classmethod
    def from_dict(cls, data):
        """Rebuild from `to_dict` output / a file header (patches/core.py:110-121): the GMM is looked up
        by name in the user's GMM library."""
        kwargs = dict(data)
        kwargs.pop("type", None)
        kwargs["gmm"] = GaussianMixtureModel.from_dict(kwargs.pop("gmm"))
        kwargs["norm"] = ImageNorm.from_dict(kwargs.pop("norm", {"type": "identity"}))
        if "patch_norm" in kwargs:
            kwargs["patch_norm"] = PatchNorm.from_dict(kwargs["patch_norm"])
        if kwargs.get("cycle_spin_subpix") and cls is GMMPatchPrior:  # (a header with PSUBSPIN = T: the subclass)
            cls = SubpixelGMMPatchPrior
        if kwargs.get("jitter") and cls is GMMPatchPrior:  # (a header with PJITTER = T: the subclass)
            cls = JitteredGMMPatchPrior
        return cls(**kwargs)


class SubpixelGMMPatchPrior(GMMPatchPrior):
    """`GMMPatchPrior` with the reference's ``cycle_spin_subpix=True``: behind the roll the normed image is shifted by a
    random sub-pixel offset (x0, y0) in [-0.5, 0.5]^2 -- the 3 x 3 stencil of bilinear weights of
    jolideco/utils/torch.py:122-143, zero outside the rolled image -- drawn per evaluation from ``generator`` after the two
    roll draws, x0 first.  A class of its own because `GMMPatchPrior(cycle_spin_subpix=True)` keeps raising; the arguments
    are `GMMPatchPrior`'s (``cycle_spin_subpix``, if given, must be true), `to_dict` writes ``cycle_spin_subpix: True``
    under the type "gmm-patches" -- what the reference writes and reads -- and `GMMPatchPrior.from_dict`, YAML and the
    FITS keyword ``PSUBSPIN`` give this class back.

    Two streaming kernels around the unchanged pass (csrc/gmm_subpix.hip); every norm, patch norm, both patch sizes and both
    modes work with it.  The prior is evaluated whole (`shardable`, `supports_fused_step`, `supports_phases` are False;
    `device_fwd_bwd_step` raises), its `draw_shifts` returns the pair ``(roll or None, (x0, y0))``
    (``shift_kind = "roll+subpixel"``), a session with it runs by-value epochs only, it has no ``compute_error``
    (`check_hessian_ones`) and cannot be the inner prior of a `MultiScalePrior`."""

    def __init__(self, gmm=None, stride=None, cycle_spin=True, cycle_spin_subpix=True, generator=None, norm=None,
                 patch_norm=None, jitter=False, marginalize=False, device=TORCH_DEFAULT_DEVICE):
        if not cycle_spin_subpix:
            raise ValueError("SubpixelGMMPatchPrior is the prior with cycle_spin_subpix=True: use GMMPatchPrior without it")
        super().__init__(gmm=gmm, stride=stride, cycle_spin=cycle_spin, generator=generator, norm=norm, patch_norm=patch_norm,
                         jitter=jitter, marginalize=marginalize, device=device)
        self.cycle_spin_subpix = True

    shift_kind = "roll+subpixel"
    _variant_keyword = "subpix"
    _variant_form = "(x0, y0)"
    # (the zero-padded stencil of a constant image is not constant at the border and the seam of the roll, so a constant
    # vector is not in the null space of the patches' quadratic forms)
    _no_hessian_ones = "cycle_spin_subpix: the Hessian product with ones is not zero behind the zero-padded sub-pixel stencil"

    def _draw_variant(self, grid):
        """(x0, y0), x0 first"""
        return subpixel_offsets(self.generator)

    @staticmethod
    def _order_variant(offsets):
        return None if offsets is None or isinstance(offsets, int) else offsets


class JitteredGMMPatchPrior(GMMPatchPrior):
    """`GMMPatchPrior` with the reference's ``jitter=True`` (jolideco/utils/torch.py:278-334): behind the norm and the roll
    every patch row and every patch column is moved by a draw of its own in [-overlap, overlap], fresh on every evaluation
    -- the reference's remedy against the block pattern of a fixed patch grid.  The grid is
    ``arange(overlap, n - stride - overlap, stride)`` per axis (`utils.torch.jitter_grid`); the draws come from
    ``generator`` after the two roll draws, the columns' first (`utils.torch.jitter_draws`), also when ``overlap == 0``.
    A class of its own because `GMMPatchPrior(jitter=True)` keeps raising; the arguments are `GMMPatchPrior`'s (``jitter``,
    if given, must be true; ``cycle_spin_subpix=True`` with it raises NotImplementedError), `to_dict` writes
    ``jitter: True`` under the type "gmm-patches" -- what the reference writes and reads -- and `GMMPatchPrior.from_dict`,
    YAML and the FITS keyword ``PJITTER`` give this class back.

    The reference keeps no patch inside the image and fails with an IndexError on an unlucky draw.  Here an image shape that
    a draw could push a patch out of is refused with a ValueError, on every evaluation path, before anything is drawn.
    Below half a patch no shape is safe, so the constructor refuses such a stride (ValueError): the stride is in [P/2, P].

    Two streaming kernels around the unchanged pass (csrc/gmm_jitter.hip); every norm, patch norm, both patch sizes and both
    modes work with it.  The prior is evaluated whole (`shardable`, `supports_fused_step`, `supports_phases` are False;
    `device_fwd_bwd_step` raises), its `draw_shifts(shape)` returns ``(roll or None, (jitter_x, jitter_y))``
    (``shift_kind = "roll+jitter"``), a session with it runs by-value epochs only, and it cannot be the inner prior of a
    `MultiScalePrior`.  ``compute_error`` works as for the plain prior: a jittered patch still has its mean subtracted."""

    def __init__(self, gmm=None, stride=None, cycle_spin=True, cycle_spin_subpix=False, generator=None, norm=None,
                 patch_norm=None, jitter=True, marginalize=False, device=TORCH_DEFAULT_DEVICE):
        if not jitter:
            raise ValueError("JitteredGMMPatchPrior is the prior with jitter=True: use GMMPatchPrior without it")
        if cycle_spin_subpix:
            raise NotImplementedError("a jittered patch grid together with cycle_spin_subpix is not implemented in jolideco_amd")
        super().__init__(gmm=gmm, stride=stride, cycle_spin=cycle_spin, generator=generator, norm=norm, patch_norm=patch_norm,
                         marginalize=marginalize, device=device)
        # (a stride outside [P / 2, P] -- given, or the mixture's ``meta.stride`` -- is refused here: no shape is safe at it)
        jitter_stride_check(max(self.patch_shape), self.stride)
        self.jitter = True

    shift_kind = "roll+jitter"
    _variant_keyword = "jitter"
    _variant_form = "(jitter_x, jitter_y)"

    def check_shape(self, shape):
        """(n_y, n_x) of the grid of an image of ``shape``; ValueError for a shape that is too small or not safe"""
        base_y, base_x = jitter_grid(shape, self.patch_shape, self.stride)
        return int(base_y.numel()), int(base_x.numel())

    def _draw_grid(self, shape):
        if shape is None:
            raise ValueError("the draw of a JitteredGMMPatchPrior depends on the image: draw_shifts(shape)")
        return self.check_shape(shape)

    def _draw_variant(self, grid):
        """(jitter_x, jitter_y): the columns' draws, then the rows', the reference's order; int64 host tensors"""
        n_y, n_x = grid
        return jitter_draws(self.generator, n_x, n_y, self.overlap)

    @staticmethod
    def _order_variant(jitter):
        """(jitter_y, jitter_x): the library's order"""
        if not (isinstance(jitter, (tuple, list)) and len(jitter) == 2 and not isinstance(jitter[0], (int, float))):
            return None
        return jitter[1], jitter[0]

    def n_patch_rows(self, shape):
        return self.check_shape(shape)[0]


MULTISCALE_MAX_LEVELS = 5  # pooling factors 1 ... 16; the widest blur has 43 taps (JD_MULTISCALE_MAX_LEVELS)


def multiscale_level_taps(level, anti_alias=True):
    """The factor u (float32 values as Python floats) of the blur of ``level``: the reference convolves with
    ``Gaussian2DKernel(sigma = 2 * 2**level / 6)`` cast to float32 (priors/patches/core.py:316-320) -- 3, 7, 11, 23, 43 pixels
    for levels 0 ... 4, an exact outer product K = u u^T with u = K[centre, :] / sqrt(K[centre, centre]).  No blur: [1]."""
    if not anti_alias:
        return [1.0]
    kernel = gaussian_kernel_2d(2 * 2**level / 6.0).astype(np.float32).astype(np.float64)
    centre = kernel.shape[0] // 2
    return [float(v) for v in (kernel[centre] / np.sqrt(kernel[centre, centre])).astype(np.float32)]


class MultiScalePrior(Prior):
    """The inner prior on a Gaussian-blurred, average-pooled pyramid of the flux (reference:
    jolideco/priors/patches/core.py:249-337; exported there, not registered, and not registered here)::

        g = flux
        for l in range(n_levels), f = 2**l:
            if w_l == 0: continue                       # (its blur is skipped too)
            if anti_alias: g = K_l (*) g                # Gaussian of sigma 2 f / 6, "same", zero padded, cumulative
            value += f**2 * w_l * prior(avg_pool2d(g, f))

    Same constructor as the reference.  ``weights`` (default 1 / n_levels each) are stored as log-weights and normalised by
    a softmax, in float32, as the reference does; they are constants of the prior here (the reference trains
    ``_log_weights``), like the parameters of the image norms.  At most 5 levels.  ``prior``: any prior of this package with a
    `device_fwd_bwd` except another `MultiScalePrior`, a `SubpixelGMMPatchPrior` (NotImplementedError:
    its draw is a roll and two offsets, not a level's roll) and a `JitteredGMMPatchPrior` (NotImplementedError: its draw
    depends on each level's shape).

    ``cycle_spin=True`` (the default): the full-resolution flux is rolled by one draw of
    ``cycle_spin_shifts(prior.patch_shape, prior.generator)`` in front of the levels -- what the reference's
    ``flux, _ = cycle_spin(...)`` means.  The reference itself raises ValueError there (`cycle_spin` returns one tensor), so
    this setting is checked against the restatement of the formula above only; ``cycle_spin=False`` is checked against
    the reference.

    The blur, the pooling and their adjoints are two HIP kernels (csrc/multiscale.hip); the levels' values are summed on
    the device.  The work buffers (two full-resolution images, the pooled image and its gradient per level, the level
    values) belong to the prior, per device and shape: after the first call for a shape nothing is allocated, and no call
    synchronises with the host.  A session with this prior runs by-value epochs only; the prior is not shardable, has no
    fused optimizer step, no phases, no ``compute_error`` and no file format.
    """

    shift_kind = "levels"  # what `draw_shifts` returns: (outer roll, one entry per level)
    shardable = False
    supports_fused_step = False
    supports_phases = False

    def __init__(self, prior, n_levels=2, weights=None, cycle_spin=True, anti_alias=True):
        super().__init__()
        if isinstance(prior, MultiScalePrior) or not isinstance(prior, Prior) or type(prior).device_fwd_bwd is Prior.device_fwd_bwd:
            raise ValueError("the inner prior must be a prior of jolideco_amd with a device_fwd_bwd, and not a MultiScalePrior")
        if getattr(prior, "shift_kind", None) == "roll+jitter":
            raise NotImplementedError(f"a MultiScalePrior around a {type(prior).__name__} is not implemented in jolideco_amd: "
                                      "the draw of a jittered patch grid depends on each level's shape")
        if getattr(prior, "shift_kind", None) == "roll+subpixel":
            raise NotImplementedError(f"a MultiScalePrior around a {type(prior).__name__} with cycle_spin_subpix is not "
                                      "implemented in jolideco_amd: its draw (roll, offsets) is not a level's roll")
        n_levels = int(n_levels)
        if not 1 <= n_levels <= MULTISCALE_MAX_LEVELS:
            raise ValueError(f"n_levels must be in [1, {MULTISCALE_MAX_LEVELS}], got {n_levels}")
        self.n_levels = n_levels
        self.cycle_spin = bool(cycle_spin)
        self.anti_alias = bool(anti_alias)
        self.prior = prior
        if self.cycle_spin and not (hasattr(prior, "patch_shape") and getattr(prior, "generator", None) is not None):
            raise ValueError("cycle_spin=True rolls by a draw of cycle_spin_shifts(prior.patch_shape, prior.generator): the "
                             f"inner {type(prior).__name__} has no patch shape / generator")
        if weights is None:
            weights = torch.tensor([1 / n_levels] * n_levels)
        weights = torch.as_tensor(weights, dtype=torch.float32).reshape(-1)
        if weights.numel() != n_levels:
            raise ValueError(f"{n_levels} levels need {n_levels} weights, got {weights.numel()}")
        if not bool(torch.all(weights >= 0)) or not bool(torch.any(weights > 0)):
            raise ValueError("weights must be non-negative and not all zero")
        self._log_weights = torch.log(weights)  # (a constant: a plain tensor, not a Parameter)
        self._taps = [multiscale_level_taps(level, self.anti_alias) for level in range(n_levels)]
        self._work = {}
        self.last_shifts = None

    def __getstate__(self):
        state = super().__getstate__()
        state["_work"] = {}
        return state

    @property
    def weights(self):
        """softmax of the log-weights, float32 (priors/patches/core.py:283-286)."""
        return torch.exp(self._log_weights) / torch.sum(torch.exp(self._log_weights))

    @property
    def patch_shape(self):
        return self.prior.patch_shape

    @property
    def levels(self):
        """[(level, f, f**2 * w_l as the reference's float32 product)] of the evaluated levels (w_l != 0), ascending."""
        return [(level, 2**level, float(2**level * 2**level * w)) for level, w in enumerate(self.weights) if w != 0]

    @property
    def _inner_draws(self):
        return hasattr(self.prior, "draw_shifts") and bool(getattr(self.prior, "draws_shifts", True))

    def draw_shifts(self):
        """One draw, in the order the reference draws: the outer roll (None when ``cycle_spin`` is off), then one entry per
        level, ascending -- the inner prior's own draw, None for a skipped level or an inner prior that draws nothing."""
        outer = cycle_spin_shifts(self.prior.patch_shape, self.prior.generator) if self.cycle_spin else None
        evaluated = {level for level, _, _ in self.levels}
        inner = tuple(self.prior.draw_shifts() if (level in evaluated and self._inner_draws) else None
                      for level in range(self.n_levels))
        self.last_shifts = (outer,) + inner
        return self.last_shifts

    def draw_shifts_many(self, n):
        return [self.draw_shifts() for _ in range(n)]

    def _buffers_for(self, flux):
        H, W = flux.shape[-2:]
        key = (str(flux.device), H, W)
        work = self._work.get(key)
        if work is None:
            patch = getattr(self.prior, "patch_shape", None)
            for level in range(self.n_levels):
                f = 2**level
                small = (H // f < 1 or W // f < 1) if patch is None else (H // f < patch[0] or W // f < patch[1])
                if small:
                    raise ValueError(f"level {level} of a {H} x {W} image is {H // f} x {W // f}: smaller than "
                                     f"{'one pixel' if patch is None else f'the inner patch {tuple(patch)}'}")
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=flux.device)  # noqa: E731
            work = self._work[key] = {
                "full": [new(H, W), new(H, W)],
                "d": [new(H // 2**level, W // 2**level) for level in range(self.n_levels)],
                "dd": [new(H // 2**level, W // 2**level) for level in range(self.n_levels)],
                "values": new(self.n_levels),
            }
        return work

    def __call__(self, flux):
        """Differentiable log-prior of a (1, 1, H, W) HIP tensor; draws once (`draw_shifts`)."""
        from ...ops import MultiScalePriorFunction

        return MultiScalePriorFunction.apply(flux, self, self.draw_shifts())

    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, shifts="draw", patch_rows=None):
        """Fused path: value -> device scalar, ``grad += coef * d logprior / d flux``.  ``shifts``: a draw of `draw_shifts`
        ("draw": drawn now).  The factors f**2 * w_l * coef travel as the inner prior's coefficient, so the pooled
        gradients arrive scaled; the weighted sum of the level values is formed on the device."""
        from ...ops import multiscale_down, multiscale_up_adjoint, multiscale_value

        if isinstance(shifts, str):
            shifts = self.draw_shifts()
        outer, inner_shifts = shifts[0], shifts[1:]
        image = flux.reshape(flux.shape[-2:])
        work = self._buffers_for(image)
        levels = self.levels
        values = work["values"][: len(levels)]
        with_grad = grad is not None
        src = image
        for i, (level, f, level_coef) in enumerate(levels):
            last = i == len(levels) - 1
            g_out = None if last else work["full"][i % 2]
            d, dd = work["d"][level], work["dd"][level]
            multiscale_down(src, f, self._taps[level], d, g_out=g_out, dd_zero=dd if with_grad else None,
                            shifts=outer if i == 0 else None)
            kwargs = {"shifts": inner_shifts[level]} if self._inner_draws else {}
            self.prior.device_fwd_bwd(d.reshape((1, 1) + tuple(d.shape)), values[i : i + 1], grad=dd if with_grad else None,
                                      coef=coef * level_coef if with_grad else 0.0, **kwargs)
            src = g_out
        coefs = [level_coef for _, _, level_coef in levels]
        if not with_grad:
            multiscale_value(values, coefs, value_out)
            return
        dg = None
        for i in range(len(levels) - 1, -1, -1):
            level, f, _ = levels[i]
            first = i == 0
            # (g_out of level i lived in full[i % 2] and is dead by now: dg_{i-1} goes to the image the level READ, never to
            # the one it takes dg_i from)
            out = grad.reshape(grad.shape[-2:]) if first else work["full"][(i + 1) % 2]
            multiscale_up_adjoint(work["dd"][level], f, self._taps[level], out, dg=dg, rolled=first,
                                  shifts=outer if first else None, value=(values, coefs, value_out) if first else None)
            dg = out

    def hessian_ones(self, flux):
        self.check_hessian_ones()

    def check_hessian_ones(self):
        """A zero-padded blur of a constant image is not constant, so the null-space argument of
        `GMMPatchPrior.hessian_ones` does not hold across the levels, and there is no kernel for the product."""
        raise NotImplementedError("compute_error=True is not implemented for a MultiScalePrior: the Hessian product with "
                                  "ones is not zero behind a zero-padded blur")

    def to_dict(self):
        """The reference's keys (priors/patches/core.py:328-337)."""
        return dict(
            n_levels=self.n_levels,
            weights=self.weights.detach().numpy().tolist(),
            cycle_spin=self.cycle_spin,
            anti_alias=self.anti_alias,
            prior=self.prior.to_dict(),
        )

"""Prior base classes and the element-wise priors (reference: jolideco/priors/core.py).

Every prior exposes two entry points:
  * ``__call__(flux) -> 0-dim tensor`` : differentiable log-prior (autograd seam, HIP backward)
  * ``device_fwd_bwd(flux, value_out, grad, coef)`` : the fused path used by the fit loop, which
    writes the value into a device scalar and accumulates ``coef * d logprior / d flux`` into
    ``grad`` without going through autograd.
"""
import math

import torch
import torch.nn as nn

from .. import _hip
from .._hip import check, ptr, stream_ptr
from ..utils.numpy import gaussian_kernel_2d
from ..utils.torch import get_default_generator, subpixel_kernel, subpixel_offsets, subpixel_offsets_many

SEPARABLE_MAX_EDGE = 68  # SEP_MAX_K of csrc/kernels.h

__all__ = ["Prior", "Priors", "UniformPrior", "InverseGammaPrior", "ExponentialPrior", "SmoothnessPrior"]


class Prior(nn.Module):
    """Prior base class"""

    # torch.Generator cannot be deep-copied / pickled: carry its state instead
    # (same work-around as jolideco/priors/core.py:28-47)
    def __getstate__(self):
        state = self.__dict__.copy()
        generator = state.pop("generator", None)
        state.pop("_handle", None)
        if generator is not None:
            state["generator"] = generator.get_state()
        return state

    def __setstate__(self, state):
        generator_state = state.pop("generator", None)
        state.pop("generator-device", None)
        if generator_state is not None:
            generator = torch.Generator(device="cpu")
            generator.set_state(generator_state)
            state["generator"] = generator
        self.__dict__ = state

    def to_dict(self):
        from . import PRIOR_REGISTRY

        for name, cls in PRIOR_REGISTRY.items():
            if isinstance(self, cls):
                return {"type": name}
        return {}

    def hessian_ones(self, flux):
        """Hessian of the log-prior times a vector of ones (what `torch.autograd.functional.vhp(..., v=ones)`
        of jolideco/loss.py:263-279 yields for this prior's term).  Zero unless the prior has curvature."""
        return torch.zeros_like(flux)

    @classmethod
    def from_dict(cls, data):
        from . import PRIOR_REGISTRY

        kwargs = dict(data)
        if "type" in kwargs:
            type_ = kwargs.pop("type")
            if type_ not in PRIOR_REGISTRY:
                raise NotImplementedError(f"prior {type_!r} is not implemented in jolideco_amd")
            return PRIOR_REGISTRY[type_].from_dict(kwargs)
        return cls(**kwargs)

    # fused path ----------------------------------------------------------------------------
    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, patch_rows=None):
        raise NotImplementedError

    #: True if the value is a sum over patch rows that can be sharded across ranks
    shardable = False


class Priors(nn.ModuleDict):
    """Dict of multiple priors"""

    def __call__(self, fluxes):
        value = 0
        for idx, prior in enumerate(self.values()):
            value = value + prior(flux=fluxes[idx])
        return value


class UniformPrior(Prior):
    """Uniform prior: log-prior 0, no gradient (jolideco/priors/core.py:110-129)."""

    def __init__(self):
        super().__init__()

    def __call__(self, flux):
        return torch.tensor(0)

    value_is_zero = True  # log-prior 0, gradient 0: a session whose slot for the value already holds 0 skips the call

    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, patch_rows=None):
        value_out.zero_()


class _ElementwisePrior(Prior):
    """``cycle_spin_subpix``: the prior is evaluated on the flux shifted by a random sub-pixel offset -- a 3 x 3 stencil
    of bilinear weights (jolideco/utils/torch.py:122-143) -- drawn per evaluation from ``generator`` (a CPU generator;
    default: torch's default seed, as the reference's)."""

    _kind = 0
    shift_kind = "subpixel"  # what `draw_shifts` returns: float offsets (x0, y0), not the integer rolls of a cycle spin

    def _init_subpix(self, cycle_spin_subpix, generator):
        self.cycle_spin_subpix = bool(cycle_spin_subpix)
        self.generator = generator if generator is not None else get_default_generator("cpu")
        if self.generator.device.type != "cpu":
            raise ValueError("the cycle-spin generator must be a CPU generator")
        self.last_shifts = None

    @property
    def draws_shifts(self):
        """True when every evaluation draws from the generator: `FitSession` plans a device slot per evaluation then."""
        return self.cycle_spin_subpix

    def _params(self):
        raise NotImplementedError

    def draw_shifts(self):
        """One pair of sub-pixel offsets (x0, y0), x first: Python floats of the float32 draws `rand(1) - 0.5`."""
        self.last_shifts = subpixel_offsets(self.generator)
        return self.last_shifts

    def draw_shifts_many(self, n):
        """The next `n` pairs, in order (an epoch's worth, `FitSession._plan_epoch`)."""
        shifts = subpixel_offsets_many(self.generator, n)
        if shifts:
            self.last_shifts = shifts[-1]
        return shifts

    def __call__(self, flux):
        from ..ops import ElementwisePriorFunction

        alpha, beta, log_const = self._params()
        shifts = self.draw_shifts() if self.cycle_spin_subpix else None
        return ElementwisePriorFunction.apply(flux, self._kind, alpha, beta, log_const, shifts)

    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, patch_rows=None, shifts="draw"):
        alpha, beta, log_const = self._params()
        n = flux.numel()
        if self.cycle_spin_subpix:
            from ..ops import elementwise_prior_subpix

            if isinstance(shifts, str):
                shifts = self.draw_shifts()
            elementwise_prior_subpix(self._kind, flux, alpha, beta, log_const, shifts, value_out, coef / n, grad)
            return
        check(
            _hip.lib().jd_elementwise_prior_fwd_bwd(
                self._kind, ptr(flux), n, alpha, beta, log_const, ptr(value_out), coef / n, ptr(grad),
                stream_ptr(flux.device),
            )
        )


class InverseGammaPrior(_ElementwisePrior):
    """Product of inverse-Gamma distributions, sparse prior for point sources
    (jolideco/priors/core.py:132-240): mean_i(-beta/x_i - (alpha+1) log x_i) + alpha log beta - lgamma(alpha)."""

    _kind = 1

    def __init__(self, alpha=10, beta=3 / 2, cycle_spin_subpix=False, generator=None):
        super().__init__()
        self.alpha = float(alpha)
        self.beta = float(beta)
        self._init_subpix(cycle_spin_subpix, generator)

    @property
    def mean(self):
        return self.beta / (self.alpha - 1)

    @property
    def mode(self):
        return self.beta / (self.alpha + 1)

    @property
    def log_constant_term(self):
        a, b = torch.tensor([self.alpha]), torch.tensor([self.beta])
        return float(a * torch.log(b) - torch.lgamma(a))

    def _params(self):
        return self.alpha, self.beta, self.log_constant_term

    def hessian_ones(self, flux):
        """The prior is a mean of element-wise terms, so its Hessian is diagonal:
        d2/dx2 (-beta/x - (alpha+1) log x) / n = (-2 beta / x^3 + (alpha+1) / x^2) / n.
        With ``cycle_spin_subpix`` one pair of offsets is drawn (as the reference's evaluation does) and the prior acts on
        s = K f: Hessian x ones = K^T (v''(s) * K 1) / n, from torch ops (not on the hot path)."""
        if not self.cycle_spin_subpix:
            return (-2.0 * self.beta / flux**3 + (self.alpha + 1.0) / flux**2) / flux.numel()
        import torch.nn.functional as F

        kernel = subpixel_kernel(*self.draw_shifts()).to(flux.device).reshape(1, 1, 3, 3)
        image = flux.reshape((1, 1) + tuple(flux.shape[-2:]))
        s = F.conv2d(image, kernel, padding="same")
        k_ones = F.conv2d(torch.ones_like(image), kernel, padding="same")
        curvature = (-2.0 * self.beta / s**3 + (self.alpha + 1.0) / s**2) * k_ones
        # K^T: cross-correlation with the flipped kernel
        return (F.conv2d(curvature, torch.flip(kernel, dims=(-2, -1)), padding="same") / flux.numel()).reshape(flux.shape)

    def to_dict(self):
        data = super().to_dict()
        data.update(alpha=self.alpha, beta=self.beta, cycle_spin_subpix=bool(self.cycle_spin_subpix))
        return data


class ExponentialPrior(_ElementwisePrior):
    """Product of exponential distributions (jolideco/priors/core.py:243-339):
    mean_i(-alpha x_i) + log alpha."""

    _kind = 2

    def __init__(self, alpha=10, cycle_spin_subpix=False, generator=None):
        super().__init__()
        self.alpha = float(alpha)
        self._init_subpix(cycle_spin_subpix, generator)

    @property
    def mean(self):
        return 1 / self.alpha

    @property
    def mode(self):
        return 0

    @property
    def log_constant_term(self):
        return float(torch.log(torch.tensor([self.alpha])))

    def _params(self):
        return self.alpha, 0.0, self.log_constant_term

    def to_dict(self):
        data = super().to_dict()
        data.update(alpha=self.alpha, cycle_spin_subpix=bool(self.cycle_spin_subpix))
        return data


class SmoothnessPrior(Prior):
    """Smoothness prior (jolideco/priors/core.py:373-396): -sum(flux * (K (*) flux)) with K a Gaussian of standard
    deviation ``width`` pixels (`gaussian_kernel_2d`), "same" zero-padded convolution; not divided by the number of
    pixels.  K is symmetric and odd-sized, so the gradient is -2 K (*) flux.  The convolution runs through the plan
    machinery of the forward model (`ConvPlan`: a Gaussian is rank 1, so "auto" takes the separable kernels; kernels
    beyond their tap limit fall to the FFT path)."""

    def __init__(self, width=2):
        super().__init__()
        self.width = width
        self.kernel_numpy = gaussian_kernel_2d(width)
        self.kernel = torch.from_numpy(self.kernel_numpy[None, None])
        self._operators = {}

    def __getstate__(self):
        state = super().__getstate__()
        state["_operators"] = {}
        return state

    def _operator(self, flux):
        """(plan, operator) of this prior's kernel for the image shape and device of ``flux`` (built once per shape)."""
        from ..ops import ConvPlan, default_conv_method, psf_separable_rank

        H, W = flux.shape[-2:]
        k = self.kernel_numpy.shape[0]
        method = default_conv_method()
        # (a plan asked for by size alone is a general kernel's: the low-rank test is the caller's, as in NPredModel --
        # a sampled Gaussian is one outer product, up to the tap limit of the separable kernels)
        if method == "auto" and k <= SEPARABLE_MAX_EDGE and psf_separable_rank(self.kernel_numpy) == 1:
            method = "separable"
        plan = ConvPlan.get(H, W, k, k, flux.device, method=method)
        key = (str(flux.device), H, W, method)
        entry = self._operators.get(key)
        if entry is None or entry[0] is not plan:
            psf = torch.from_numpy(self.kernel_numpy.astype("float32")).to(flux.device)
            entry = self._operators[key] = (plan, plan.psf_spectrum(psf))
        return entry

    def __call__(self, flux):
        from ..ops import SmoothnessPriorFunction

        plan, khat = self._operator(flux)
        return SmoothnessPriorFunction.apply(flux, plan, khat)

    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, patch_rows=None):
        from ..ops import smoothness_prior

        plan, khat = self._operator(flux)
        smoothness_prior(plan, khat, flux, value_out, coef, grad)

    def hessian_ones(self, flux):
        """The log-prior is the quadratic form -f^T K f: Hessian x ones = -2 K (*) 1."""
        plan, khat = self._operator(flux)
        return -2.0 * plan.conv_same(torch.ones_like(flux).contiguous(), None, khat).reshape(flux.shape)

    def to_dict(self):
        data = super().to_dict()
        data["width"] = float(self.width)
        return data

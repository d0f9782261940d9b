"""Image / patch normalisations used by the GMM patch prior.

Image norms (reference jolideco/utils/norms.py:225-426): identity, asinh, fixed-max, sigmoid, atan, log and power.  On
the device the norm is one streaming pass in front of the patch kernels and its derivative rides in the gather kernel
(csrc/gmm_gather.hip); the classes here carry the parameters, the plain-torch evaluation (any device) and the (de)serialisation.
``"max"`` (a global reduction) and ``"inverse-cdf"`` (a table lookup) are not implemented and raise NotImplementedError.
Patch norms (:97-112): `SubtractMeanPatchNorm` and `StandardizedSubtractMeanPatchNorm`, both fused into the dense HIP
kernels (`device_kind` selects the instantiation, jd_gmm_set_patch_norm).
"""
import numpy as np
import torch

__all__ = [
    "PatchNorm",
    "SubtractMeanPatchNorm",
    "StandardizedSubtractMeanPatchNorm",
    "ImageNorm",
    "IdentityImageNorm",
    "ASinhImageNorm",
    "FixedMaxImageNorm",
    "SigmoidImageNorm",
    "ATanImageNorm",
    "LogImageNorm",
    "PowerImageNorm",
    "NORMS_REGISTRY",
    "NORMS_PATCH_REGISTRY",
]


class PatchNorm:
    """Patch normalisation base class"""

    #: kind of `jd_gmm_set_patch_norm` (include/jolideco_hip.h); None: no device kernel
    device_kind = None

    def to_dict(self):
        for name, cls in NORMS_PATCH_REGISTRY.items():
            if isinstance(self, cls):
                return {"type": name}
        return {}

    @classmethod
    def from_dict(cls, data):
        kwargs = dict(data)
        if "type" in kwargs:
            type_ = kwargs.pop("type")
            if type_ not in NORMS_PATCH_REGISTRY:
                raise NotImplementedError(f"patch norm {type_!r} is not implemented in jolideco_amd")
            return NORMS_PATCH_REGISTRY[type_](**kwargs)
        return cls(**kwargs)


class SubtractMeanPatchNorm(PatchNorm):
    """Subtract the patch mean (Zoran & Weiss).  On device this is fused into the GMM kernel
    (csrc/gmm_gather.hip); this host version works on torch tensors for explicit patch arrays."""

    device_kind = 0

    def __call__(self, patches):
        return patches - patches.nanmean(dim=1, keepdim=True)


class StandardizedSubtractMeanPatchNorm(PatchNorm):
    """Relative contrast of a patch: subtract the patch mean, then divide by it (reference utils/norms.py:106-112).  On
    the device it is fused into the dense fp32 GMM kernels (csrc/gmm_dense.hip, csrc/gmm256.hip), which a prior with
    this norm always takes; this host version works on torch tensors for explicit patch arrays."""

    device_kind = 1

    def __call__(self, patches):
        patches_mean = patches.nanmean(dim=1, keepdim=True)
        return (patches - patches_mean) / patches_mean


class ImageNorm:
    """Image normalisation base class.

    One deliberate deviation from the reference: there the parameters of a norm (alpha, beta, max_value) are
    ``nn.Parameter``s that reach the optimizer through ``nn.Module.parameters`` unless the norm is ``frozen``.  Here they
    are CONSTANTS of the prior -- float32 tensors without gradient, handed to the kernels by value (a captured epoch
    bakes them in).  ``frozen`` is accepted and stored and has no other effect; results equal the reference's with the
    norm's parameters set to ``requires_grad_(False)``.
    """

    #: kind of `jd_image_norm` (include/jolideco_hip.h); None: no device kernel
    device_kind = None

    def __init__(self, frozen=False):
        self.frozen = frozen

    def device_params(self):
        """(kind, p0, p1) of `jd_image_norm`."""
        return self.device_kind, 0.0, 0.0

    def to_dict(self):
        for name, cls in NORMS_REGISTRY.items():
            if isinstance(self, cls):
                return {"type": name}
        return {}

    @classmethod
    def from_dict(cls, data):
        kwargs = dict(data)
        if "type" in kwargs:
            type_ = kwargs.pop("type")
            if type_ not in NORMS_REGISTRY:
                raise NotImplementedError(f"image norm {type_!r} is not implemented in jolideco_amd")
            return NORMS_REGISTRY[type_](**kwargs)
        return cls(**kwargs)

    def __call__(self, image):
        raise NotImplementedError

    def inverse(self, image):
        raise NotImplementedError

    def evaluate_numpy(self, image):
        """Evaluate the norm on a numpy array (float32, as the reference)"""
        image = torch.from_numpy(np.asarray(image).astype(np.float32))
        return self(image).detach().numpy()

    def inverse_numpy(self, image):
        """Evaluate the inverse norm on a numpy array"""
        image = torch.from_numpy(np.asarray(image).astype(np.float32))
        return self.inverse(image).detach().numpy()

    @staticmethod
    def _constant(value):
        # (1,) float32, as the reference's torch.Tensor([value]): the same rounding of the parameter
        return torch.tensor([float(value)], dtype=torch.float32)

    def _p(self, name, image):
        value = getattr(self, name)
        return value if value.device == image.device else value.to(image.device)


class IdentityImageNorm(ImageNorm):
    """Identity image norm"""

    device_kind = 0

    def __call__(self, image):
        return image

    def inverse(self, image):
        return image


class ASinhImageNorm(ImageNorm):
    """Inverse hyperbolic sine image norm: asinh(f / alpha) / asinh(beta / alpha)"""

    device_kind = 1

    def __init__(self, alpha=1.0, beta=1.0, **kwargs):
        super().__init__(**kwargs)
        self.alpha = self._constant(alpha)
        self.beta = self._constant(beta)

    def device_params(self):
        return self.device_kind, float(self.alpha), float(self.beta)

    def __call__(self, image):
        alpha, beta = self._p("alpha", image), self._p("beta", image)
        top = torch.asinh(image / alpha)
        bottom = torch.asinh(beta / alpha)
        return top / bottom

    def inverse(self, image):
        alpha, beta = self._p("alpha", image), self._p("beta", image)
        value = image * torch.asinh(beta / alpha)
        return alpha * torch.sinh(value)

    def to_dict(self):
        data = super().to_dict()
        data["alpha"] = float(self.alpha)
        data["beta"] = float(self.beta)
        return data


class FixedMaxImageNorm(ImageNorm):
    """Fixed max image normalisation: clip(f / max_value, 0, 1)"""

    device_kind = 2

    def __init__(self, max_value, **kwargs):
        super().__init__(**kwargs)
        self.max_value = self._constant(max_value)

    def device_params(self):
        return self.device_kind, float(self.max_value), 0.0

    def __call__(self, image):
        return torch.clip(image / self._p("max_value", image), min=0, max=1)

    def inverse(self, image):
        return image * self._p("max_value", image)

    def to_dict(self):
        data = super().to_dict()
        data["max_value"] = float(self.max_value)
        return data


class SigmoidImageNorm(ImageNorm):
    """Sigmoid image normalisation: 1 / (1 + exp(-(f - beta / 2) / alpha))"""

    device_kind = 3

    def __init__(self, alpha=1, beta=1.0, **kwargs):
        super().__init__(**kwargs)
        self.alpha = self._constant(alpha)
        self.beta = self._constant(beta)

    def device_params(self):
        return self.device_kind, float(self.alpha), float(self.beta)

    def __call__(self, image):
        alpha, beta = self._p("alpha", image), self._p("beta", image)
        return 1 / (1 + torch.exp(-(image - beta / 2.0) / alpha))

    def inverse(self, image):
        alpha, beta = self._p("alpha", image), self._p("beta", image)
        return alpha * torch.log(image / (1.0 - image)) + beta / 2.0

    def to_dict(self):
        data = super().to_dict()
        data["alpha"] = float(self.alpha)
        data["beta"] = float(self.beta)
        return data


class ATanImageNorm(ImageNorm):
    """ATan image normalisation: 2 atan(f / alpha) / pi"""

    device_kind = 4

    def __init__(self, alpha=1, **kwargs):
        super().__init__(**kwargs)
        self.alpha = self._constant(alpha)

    def device_params(self):
        return self.device_kind, float(self.alpha), 0.0

    def __call__(self, image):
        return 2 * torch.atan(image / self._p("alpha", image)) / torch.pi

    def inverse(self, image):
        return 0.5 * torch.pi * torch.tan(image)  # (as the reference: without alpha)

    def to_dict(self):
        data = super().to_dict()
        data["alpha"] = float(self.alpha)
        return data


class LogImageNorm(ImageNorm):
    """Log image normalisation: log(f / alpha)"""

    device_kind = 5

    def __init__(self, alpha=1, **kwargs):
        super().__init__(**kwargs)
        self.alpha = self._constant(alpha)

    def device_params(self):
        return self.device_kind, float(self.alpha), 0.0

    def __call__(self, image):
        return torch.log(image / self._p("alpha", image))

    def inverse(self, image):
        return self._p("alpha", image) * torch.exp(image)

    def to_dict(self):
        data = super().to_dict()
        data["alpha"] = float(self.alpha)
        return data


class PowerImageNorm(ImageNorm):
    """Power image normalisation: (f / beta)^alpha"""

    device_kind = 6

    def __init__(self, alpha=1, beta=1, **kwargs):
        super().__init__(**kwargs)
        self.alpha = self._constant(alpha)
        self.beta = self._constant(beta)

    def device_params(self):
        return self.device_kind, float(self.alpha), float(self.beta)

    def __call__(self, image):
        return torch.pow(image / self._p("beta", image), self._p("alpha", image))

    def inverse(self, image):
        return self._p("beta", image) * torch.pow(image, 1 / self._p("alpha", image))

    def to_dict(self):
        data = super().to_dict()
        data["alpha"] = float(self.alpha)
        data["beta"] = float(self.beta)
        return data


NORMS_REGISTRY = {
    "fixed-max": FixedMaxImageNorm,
    "sigmoid": SigmoidImageNorm,
    "atan": ATanImageNorm,
    "asinh": ASinhImageNorm,
    "log": LogImageNorm,
    "power": PowerImageNorm,
    "identity": IdentityImageNorm,
}
NORMS_PATCH_REGISTRY = {
    "std-subtract-mean": StandardizedSubtractMeanPatchNorm,
    "subtract-mean": SubtractMeanPatchNorm,
}

from .core import ExponentialPrior, InverseGammaPrior, Prior, Priors, SmoothnessPrior, UniformPrior
from .patches import GaussianMixtureModel, GMMPatchPrior, JitteredGMMPatchPrior, MultiScalePrior, SubpixelGMMPatchPrior

PRIOR_REGISTRY = {
    "uniform": UniformPrior,
    "gmm-patches": GMMPatchPrior,
    "inverse-gamma": InverseGammaPrior,
    "exponential": ExponentialPrior,
    "smooth": SmoothnessPrior,
}

__all__ = [
    "GaussianMixtureModel",
    "GMMPatchPrior",
    "MultiScalePrior",
    "SubpixelGMMPatchPrior",
    "JitteredGMMPatchPrior",
    "ExponentialPrior",
    "UniformPrior",
    "InverseGammaPrior",
    "SmoothnessPrior",
    "Prior",
    "Priors",
    "PRIOR_REGISTRY",
]

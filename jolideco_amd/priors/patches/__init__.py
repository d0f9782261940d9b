from .core import GMMPatchPrior, MultiScalePrior
from .gmm import GaussianMixtureModel, GaussianMixtureModelMeta

__all__ = ["GMMPatchPrior", "MultiScalePrior", "GaussianMixtureModel", "GaussianMixtureModelMeta"]

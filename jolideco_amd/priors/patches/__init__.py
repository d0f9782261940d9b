from .core import GMMPatchPrior, MultiScalePrior, SubpixelGMMPatchPrior
from .gmm import GaussianMixtureModel, GaussianMixtureModelMeta
from .kmeans import KMeansResult, kmeans, kmeans_plusplus

__all__ = ["GMMPatchPrior", "SubpixelGMMPatchPrior", "MultiScalePrior", "GaussianMixtureModel", "GaussianMixtureModelMeta", "kmeans", "kmeans_plusplus",
           "KMeansResult"]

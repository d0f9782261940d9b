from .core import GMMPatchPrior, JitteredGMMPatchPrior, MultiScalePrior, SubpixelGMMPatchPrior
from .gmm import GaussianMixtureModel, GaussianMixtureModelMeta
from .kmeans import KMeansResult, kmeans, kmeans_plusplus

__all__ = ["GMMPatchPrior", "SubpixelGMMPatchPrior", "JitteredGMMPatchPrior", "MultiScalePrior", "GaussianMixtureModel", "GaussianMixtureModelMeta", "kmeans", "kmeans_plusplus",
           "KMeansResult"]

from .core import GMMPatchPrior, MultiScalePrior
from .gmm import GaussianMixtureModel, GaussianMixtureModelMeta
from .kmeans import KMeansResult, kmeans, kmeans_plusplus

__all__ = ["GMMPatchPrior", "MultiScalePrior", "GaussianMixtureModel", "GaussianMixtureModelMeta", "kmeans", "kmeans_plusplus",
           "KMeansResult"]

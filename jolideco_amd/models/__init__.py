from .core import FluxComponents, SparseSpatialFluxComponent, SpatialFluxComponent
from .npred import NPredCalibration, NPredCalibrations, NPredModel, NPredModels

__all__ = ["FluxComponents", "SpatialFluxComponent", "SparseSpatialFluxComponent", "NPredModel", "NPredModels", "NPredCalibration", "NPredCalibrations"]

"""Inputs shared by tests/test_mixed_upsampling_golden.py (CPU) and tests/test_gpu_mixed_upsampling.py (GPU): host arrays
only, nothing here touches a device."""
import numpy as np


def clip_case():
    """One dataset on a 64 x 72 counts grid, factors (1, 2), whose "points" PSF has negative lobes (a sharpening kernel:
    narrow Gaussian minus a wider one, unit sum) on a spiky flux: a fair share of its pooled pixels is below zero
    (checked on the CPU in tests/test_mixed_upsampling_golden.py).  Returns (dataset, [flux_extended, flux_points] on
    their own grids, factors)."""
    from jolideco_amd.data import gaussian_kernel

    rs = np.random.RandomState(17)
    shape, ups = (64, 72), (1, 2)
    lobed = 2.2 * gaussian_kernel(0.8, (7, 7)) - 1.2 * gaussian_kernel(2.0, (7, 7))
    assert lobed.min() < 0 and abs(lobed.sum() - 1.0) < 1e-6
    exposure = (1 + 0.3 * np.linspace(-1, 1, shape[0])).reshape(-1, 1) * np.ones(shape)
    data = {
        "counts": rs.poisson(3.0, size=shape).astype(np.float32),
        "psf": {"extended": gaussian_kernel(1.5, (9, 9)).astype(np.float32), "points": lobed.astype(np.float32)},
        "exposure": exposure.astype(np.float32),
        "background": np.full(shape, 0.4, np.float32),
    }
    flux_ext = rs.gamma(30, size=shape).astype(np.float32) * 0.05
    flux_pts = (rs.gamma(0.15, size=(shape[0] * 2, shape[1] * 2)) * 2.0).astype(np.float32) + 1e-3
    return data, [flux_ext, flux_pts], ups

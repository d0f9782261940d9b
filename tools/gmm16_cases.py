"""Shared by tools/make_golden_gmm16.py, tests/test_gmm16_golden.py (CPU) and tests/test_gpu_gmm16.py (GPU), which import
it as `tools.gmm16_cases` with the repository root on the path: the inputs of
the 16x16 (256-feature) GMM patch prior cases and their oracle, `oracle/cpu_ref` (pinned against the live reference
when tools/make_golden_gmm16.py generated tests/golden/gmm16.npz).

The mixtures are synthetic and never stored: `cpu_ref.synthetic_gmm(K, 256, seed, zero_means=False)` rounded to float32,
rebuilt here from (K, seed); the fixture holds a float64 checksum of the ones it was generated with."""
import functools

import numpy as np
import torch

from oracle import cpu_ref

D = 256
K, SEED, STRIDE = 5, 1601, 8
SHAPE = (48, 56)
FILTERED_PIXEL = (2, 3)  # covered by patch (0, 0) only at stride 8: exactly one patch is filtered
ASINH = {"alpha": 3.0, "beta": 40.0}
FIT_SHAPE, FIT_EPOCHS, FIT_SEED, FIT_K, FIT_GMM_SEED = (48, 48), 6, 77, 4, 1603


@functools.lru_cache(maxsize=None)
def synthetic_mixture(k, seed):
    """(means, covariances, weights) as float64 arrays holding float32 values"""
    arrays = cpu_ref.synthetic_gmm(k, D, seed=seed, zero_means=False)
    return tuple(np.asarray(a, dtype=np.float32).astype(np.float64) for a in arrays)


def mixture_checksum(arrays):
    means, covs, weights = arrays
    ramp = 1.0 + np.arange(covs.size, dtype=np.float64).reshape(covs.shape) / covs.size  # (position sensitive)
    return float(np.sum(covs * ramp) + np.sum(means) + np.sum(weights * np.arange(1, weights.size + 1)))


def fixture_flux(filtered=True):
    flux = np.random.RandomState(1600).gamma(20, size=SHAPE).astype(np.float32)
    if filtered:
        flux[FILTERED_PIXEL] = -2e5
    return flux


def case_flux(shape, seed):
    return np.random.RandomState(seed).gamma(20, size=shape).astype(np.float32)


def mean_free_patches(flux, stride):
    """(N, 256) float32: every 16x16 patch minus its mean"""
    x = cpu_ref.overlapping_patches(torch.from_numpy(np.asarray(flux, dtype=np.float32)), 16, stride)
    return (x - x.mean(dim=1, keepdim=True)).numpy()


def n_patches(shape, stride):
    return ((shape[0] - 16) // stride + 1) * ((shape[1] - 16) // stride + 1)


def dense_factors(arrays, seed, amplitude=0.05):
    """(K, 256, 256) float32 factors that are NOT triangular: the precision Cholesky factors of the mixture plus a seeded
    strictly lower triangular perturbation (relative to each factor's mean |diagonal|).  Not the factor of any
    covariance -- the log-probability formula takes any matrix with a positive diagonal, in the library as in the
    oracle, and that is all the dense kernels need to be compared on."""
    pc = cpu_ref.precision_cholesky(arrays[1]).astype(np.float32)
    rs = np.random.RandomState(seed)
    for k in range(pc.shape[0]):
        scale = amplitude * np.abs(np.diag(pc[k])).mean() / 16.0
        pc[k] += np.tril(rs.normal(size=pc[k].shape), -1).astype(np.float32) * np.float32(scale)
    return pc


def oracle(flux_np, arrays, stride, shifts, marginalize, dtype=np.float32, norm=None, meta_stride=STRIDE, factors=None):
    """Sum over the kept patches of the per-patch value (max | logsumexp over the components) of `norm(flux)` and its
    gradient with respect to the raw flux (autograd), in `dtype`.  Returns a dict: total, grad (float64 array), keep
    (bool per patch of the rolled frame's grid), loglike ((kept, K) float64), and in max mode arg (int per patch, -1 for
    a filtered one) and margin (best minus runner-up per patch, inf for K = 1 or a filtered patch).
    The prior is `total * stride^2 / 256 / numel`.  `factors`: see `dense_factors`."""
    shifts = None if shifts is None else (int(shifts[0]), int(shifts[1]))
    with cpu_ref.precision(dtype):
        if factors is None:
            gmm = cpu_ref.GMM.from_numpy(*arrays, stride=meta_stride)
        else:  # explicit (not triangular) factors in place of the Cholesky factors of the covariances
            gmm = cpu_ref.GMM(means=cpu_ref._tensor(arrays[0]), precisions_cholesky=cpu_ref._tensor(factors),
                              weights=cpu_ref._tensor(arrays[2]), stride=meta_stride)
        flux = cpu_ref._tensor(flux_np[np.newaxis, np.newaxis]).requires_grad_(True)
        image = flux if norm is None else norm(flux)
        loglike = cpu_ref.gmm_patch_log_like(image, gmm, stride, shifts)
        rolled = image.detach() if shifts is None else torch.roll(image.detach(), shifts=shifts, dims=(2, 3))
        keep = torch.all(cpu_ref.overlapping_patches(rolled, 16, stride) > -1e5, dim=1).numpy()
        out = {"keep": keep, "loglike": loglike.detach().numpy().astype(np.float64)}
        if marginalize:
            values = torch.logsumexp(loglike, dim=1)
        else:
            values = torch.max(loglike, dim=1).values
            arg = np.full(keep.size, -1, dtype=np.int32)
            arg[keep] = torch.max(loglike, dim=1).indices.numpy()
            margin = np.full(keep.size, np.inf)
            if loglike.shape[1] > 1:
                top = torch.topk(loglike, 2, dim=1).values.detach().numpy().astype(np.float64)
                margin[keep] = top[:, 0] - top[:, 1]
            out["arg"], out["margin"] = arg, margin
        total = torch.sum(values)
        total.backward()
        out["total"], out["grad"] = float(total.detach()), flux.grad.numpy()[0, 0].astype(np.float64)
        return out


def prior_scale(shape, stride):
    return stride**2 / 256.0 / (shape[0] * shape[1])

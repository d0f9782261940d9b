"""Shared by tests/test_image_norm_golden.py (CPU) and tests/test_gpu_image_norm.py (GPU): the image-norm cases of the
GMM patch prior and their oracle, `oracle/cpu_ref` on `norm(flux)` with the host norm classes (pinned against the live
reference when tools/make_golden_image_norm.py generated tests/golden/image_norm.npz)."""
import functools

import numpy as np
import torch

from oracle import cpu_ref

# type -> constructor arguments: those of the fixture (tools/make_golden_image_norm.py)
NORM_CASES = {
    "asinh": {"alpha": 3.0, "beta": 40.0},
    "fixed-max": {"max_value": 24.0},
    "sigmoid": {"alpha": 6.0, "beta": 40.0},
    "atan": {"alpha": 15.0},
    "log": {"alpha": 2.5},
    "power": {"alpha": 0.6, "beta": 30.0},
}
# (shape, stride, shifts): vector paths | W % 4 != 0: scalar paths of the norm kernel and the gather | per-pixel gather |
# one patch row per tile row
SHAPE_CASES = [((40, 44), 4, (2, -1)), ((37, 41), 4, (-1, 2)), ((40, 44), 3, (1, 1)), ((40, 44), 8, (0, -2))]
GMM_META_STRIDE = 4  # the mixture's pixel weights (GaussianMixtureModelMeta.stride); the prior's stride varies
NEAR_TIE = 1e-3      # float64 margin between the two best components below which a patch may be left out (max mode)


def make_norm(type_, **overrides):
    from jolideco_amd.utils.norms import NORMS_REGISTRY

    return NORMS_REGISTRY[type_](**dict(NORM_CASES[type_], **overrides))


def case_flux(index):
    shape = SHAPE_CASES[index][0]
    return np.random.RandomState(2310 + index).gamma(20, size=shape).astype(np.float32)


def fixture_gmm(golden, prefix="gmm/"):
    g = golden("image_norm")
    return tuple(np.asarray(g[f"{prefix}{name}"], dtype=np.float64) for name in ("means", "covariances", "weights"))


def oracle(flux_np, norm, gmm_arrays, stride, shifts, marginalize, dtype=np.float32):
    """sum over the patches of the prior's per-patch value on norm(flux) and its gradient with respect to the RAW flux
    (autograd), in `dtype`; max mode: also the arg-max per patch and the margin to the second-best component.
    The prior is `sum * stride^2 / 64 / numel`.

    float64 as arbiter: the norm's parameters are the float32 values the kernels get, and the host classes combine them
    in float32 before the image promotes the result -- for asinh the denominator asinh(beta / alpha) is a float32 number
    (a constant relative scale of up to 6e-8 on the normed image against an all-float64 evaluation; every other norm
    divides the float64 image by the parameter directly).  Far below the 3e-6 / 1e-5 floors the arbiter is used at."""
    with cpu_ref.precision(dtype):
        gmm = cpu_ref.GMM.from_numpy(*gmm_arrays, stride=GMM_META_STRIDE)
        flux = cpu_ref._tensor(flux_np[np.newaxis, np.newaxis]).requires_grad_(True)
        loglike = cpu_ref.gmm_patch_log_like(norm(flux), gmm, stride, shifts)
        arg = margin = None
        if marginalize:
            values = torch.logsumexp(loglike, dim=1)
        else:
            top = torch.topk(loglike, 2, dim=1)
            values, arg = top.values[:, 0], torch.max(loglike, dim=1).indices.numpy().astype(np.int32)
            margin = (top.values[:, 0] - top.values[:, 1]).detach().numpy().astype(np.float64)
        total = torch.sum(values)
        total.backward()
        return float(total.detach()), flux.grad.numpy()[0, 0].astype(np.float64), arg, margin


@functools.lru_cache(maxsize=None)
def _cached(type_, index, marginalize, dtype_name, gmm_key):
    shape, stride, shifts = SHAPE_CASES[index]
    return oracle(case_flux(index), make_norm(type_), _GMMS[gmm_key], stride, shifts, marginalize, np.dtype(dtype_name).type)


_GMMS = {}


def cached_oracle(golden, type_, index, marginalize, dtype):
    """`oracle` of (norm type, SHAPE_CASES[index]) on the fixture's mixture, computed once per session"""
    _GMMS.setdefault("fixture", fixture_gmm(golden))
    return _cached(type_, index, bool(marginalize), np.dtype(dtype).name, "fixture")


def rel_err(got, ref, keep=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    diff = np.abs(got - ref)
    return float((diff if keep is None else diff[keep]).max() / np.abs(ref).max())

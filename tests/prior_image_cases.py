"""Shared by tests/test_prior_image_host.py (CPU) and tests/test_gpu_prior_image.py (GPU): the cases of
`GMMPatchPrior.prior_image` and the host restatement of its formula.  Nothing here touches a device.

The reference's method (jolideco/priors/patches/core.py:123-151) cannot run as written -- it unpacks three values from
`_evaluate_log_like`, which returns one -- so there is no live-reference fixture; the yardstick is the formula its lines
state, restated from pieces this repository already trusts: `cpu_ref.gmm_patch_log_like` (pinned against the live
reference), `reconstruct_from_overlapping_patches` / `get_pixel_weights`, `np.roll` and the host `inverse_numpy` of the norms.
"""
import functools

import numpy as np
import torch

from image_norm_cases import GMM_META_STRIDE, NEAR_TIE, fixture_gmm, make_norm  # noqa: F401  (NEAR_TIE: the tests' margin)
from jolideco_amd.utils.norms import IdentityImageNorm
from jolideco_amd.utils.numpy import reconstruct_from_overlapping_patches
from oracle import cpu_ref
from tools import gmm16_cases

TILE = (16, 64)  # (rows, columns) of a tile of gmm_prior_image_gather_kernel (csrc/gmm_prior_image.hip: PI_TY, PI_TX)

# name -> (patch edge, shape, stride, roll, norm type or None)
CASES = {
    "s4-roll-a": (8, (40, 44), 4, (2, -1), None),
    "s4-roll-b": (8, (40, 44), 4, (-2, 2), None),
    "s4-no-roll": (8, (40, 44), 4, None, None),
    "s2": (8, (40, 44), 2, (1, -2), None),
    "s6": (8, (40, 44), 6, (-1, 1), None),
    "uncovered": (8, (43, 50), 4, (2, 1), None),  # rows 40 .. 42 and columns 48, 49 of the rolled frame: no patch
    "tiles": (8, (37, 150), 4, (-1, 2), None),    # 3 x 3 tiles, the last of each axis ragged (5 rows, 22 columns)
    "p16-roll-a": (16, (40, 44), 8, (4, -3), None),
    "p16-roll-b": (16, (40, 44), 8, (-4, 0), None),
}
NORM_TYPES = ("asinh", "fixed-max", "sigmoid", "atan", "log", "power")
for _type in NORM_TYPES:  # every image norm kind on one 8x8 case
    CASES[f"norm-{_type}"] = (8, (40, 44), 4, (2, -1), _type)

TABLE_SEED = 2711
# Amplitude of the seeded table: of the order of the flux's spread (gamma(20): standard deviation 4.5) under the identity;
# under a norm small against the normed image, so that R stays where every inverse is finite (sigmoid: inside (0, 1), power:
# positive, atan: below pi / 2)
TABLE_SCALE, TABLE_SCALE_NORMED = 3.0, 0.02


def case_flux(name):
    shape = CASES[name][1]
    return np.random.RandomState(2700 + sorted(CASES).index(name)).gamma(20, size=shape).astype(np.float32)


def case_norm(name):
    type_ = CASES[name][4]
    return IdentityImageNorm() if type_ is None else make_norm(type_)


def case_table(name, n_components):
    """Seeded (K, P, P) float64 table holding float32 values: unlike the eigen-images it has no sign convention"""
    patch, norm_type = CASES[name][0], CASES[name][4]
    scale = TABLE_SCALE if norm_type is None else TABLE_SCALE_NORMED
    table = np.random.RandomState(TABLE_SEED).normal(size=(n_components, patch, patch)) * scale
    return table.astype(np.float32).astype(np.float64)


def mixture(golden, patch):
    """(means, covariances, weights, meta stride): the K = 12 8x8 mixture of tests/golden/image_norm.npz | the synthetic
    16x16 mixture of tools/gmm16_cases.py"""
    if patch == 8:
        return fixture_gmm(golden) + (GMM_META_STRIDE,)
    return gmm16_cases.synthetic_mixture(gmm16_cases.K, gmm16_cases.SEED) + (gmm16_cases.STRIDE,)


def n_patches(shape, stride, patch):
    return (shape[0] - patch) // stride + 1, (shape[1] - patch) // stride + 1


def restated(flux, norm, gmm_arrays, stride, roll, table, dtype, meta_stride=GMM_META_STRIDE):
    """(image, arg-max per patch, margin between the two best components per patch) of the formula in `dtype`:
    N = norm(flux), R0 = roll(N, roll); per patch of the plain prior's grid the mean m and the arg-max k of the mean-free
    patch's log-likelihood; R = the weighted overlap-add of table[k] + m; image = norm.inverse(roll(R, -roll)).  The
    arg-max and the margin are meaningful in float64, where the tests take them from."""
    patch = table.shape[-1]
    shape = flux.shape
    with cpu_ref.precision(dtype):
        gmm = cpu_ref.GMM.from_numpy(*gmm_arrays, stride=meta_stride)
        normed = norm(cpu_ref._tensor(flux[np.newaxis, np.newaxis]))
        loglike = cpu_ref.gmm_patch_log_like(normed, gmm, stride, roll)
        rolled = normed if roll is None else torch.roll(normed, shifts=roll, dims=(2, 3))
        means = cpu_ref.overlapping_patches(rolled, patch, stride).mean(dim=1).numpy()
        top = torch.topk(loglike, 2, dim=1)
        arg = torch.max(loglike, dim=1).indices.numpy()
        margin = (top.values[:, 0] - top.values[:, 1]).numpy().astype(np.float64)
    n_y, n_x = n_patches(shape, stride, patch)
    assert loglike.shape[0] == n_y * n_x == means.size, "a filtered patch: the restatement has no rule for it"
    patches = table.astype(dtype)[arg] + means.astype(dtype).reshape((-1, 1, 1))
    reco = reconstruct_from_overlapping_patches(patches=patches, image_shape=shape, stride=stride)
    if roll is not None:
        reco = np.roll(reco, shift=(-roll[0], -roll[1]), axis=(0, 1))
    return norm.inverse_numpy(reco.astype(dtype)).astype(np.float64), arg.astype(np.int32), margin


_GOLDEN = {}


@functools.lru_cache(maxsize=None)
def _cached(name, dtype_name):
    patch, shape, stride, roll, _ = CASES[name]
    *arrays, meta_stride = mixture(_GOLDEN["load"], patch)
    table = case_table(name, arrays[0].shape[0])
    return restated(case_flux(name), case_norm(name), tuple(arrays), stride, roll, table, np.dtype(dtype_name).type, meta_stride)


def cached_restated(golden, name, dtype):
    """`restated` of a case with its seeded table, computed once per session; the result is shared: do not write to it"""
    _GOLDEN.setdefault("load", golden)
    return _cached(name, np.dtype(dtype).name)


def kept_pixels(margin, name):
    """(pixels left in the comparison, clear patches): a patch whose float64 margin is below NEAR_TIE is a near tie, and
    the pixels it covers -- un-rolled frame -- are left out"""
    from conftest import patch_cover_mask

    patch, shape, stride, roll, _ = CASES[name]
    clear = np.asarray(margin) >= NEAR_TIE
    return ~patch_cover_mask(np.flatnonzero(~clear), shape, stride, roll, patch=patch), clear


def weight_sum(shape, stride, patch):
    """Sum of the pixel weights of the patches covering each pixel: what a zero table and a constant flux reconstruct"""
    n_y, n_x = n_patches(shape, stride, patch)
    return reconstruct_from_overlapping_patches(np.ones((n_y * n_x, patch, patch)), shape, stride)

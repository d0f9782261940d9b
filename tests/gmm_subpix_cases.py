"""Shared by tools/make_golden_gmm_subpix.py, tests/test_gmm_subpix_golden.py (CPU) and tests/test_gpu_gmm_subpix.py
(GPU): the cases of the GMM patch prior with a sub-pixel cycle spin (`cycle_spin_subpix=True`) and their oracle.

The oracle restates the reference (jolideco/priors/patches/core.py:189-246, utils/torch.py:31-38,91-143) from torch and
`oracle/cpu_ref`: n = norm(flux), `torch.roll`, `F.conv2d(., k, padding="same")` with the float32 weights of
`grid_weights`, then the patch log-likelihoods of `cpu_ref`, max or logsumexp, the sum, autograd.  It was pinned against the
live reference when tools/make_golden_gmm_subpix.py generated tests/golden/gmm_subpix.npz."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import image_norm_cases
import patch_norm_cases
import prior_cases
from oracle import cpu_ref
from tools import gmm16_cases

NEAR_TIE = image_norm_cases.NEAR_TIE  # float64 margin between the two best components below which a patch is a near tie
TILE = (16, 64)  # rows x columns of a tile of the two kernels (GS_TY x GS_TX of csrc/gmm_subpix.hip)

# (shape, stride, roll, offsets (x0, y0)) on 8 x 8 patches.  Shapes: vector paths | W % 4 != 0: scalar paths | stride that
# does not divide the patch | one patch row per 8 rows, odd width | every pixel within one of a border or the seam | more than
# one tile in both directions (5 x 2 tiles of TILE).  Rolls: None, (0, 0), negative, mixed sign.  Offsets: generic, (0, 0),
# the four corners (two weights of 0.5 per direction, the `< 1` cut drops the third).
CASES = [
    ((40, 44), 4, (2, -1), (0.3, -0.2)),
    ((40, 44), 4, None, (-0.5, 0.5)),
    ((37, 41), 4, (-1, 2), (-0.25, 0.4)),
    ((37, 41), 4, (0, 0), (0.5, 0.5)),
    ((40, 44), 3, (1, 1), (0.0, 0.0)),
    ((24, 27), 8, (-2, -2), (0.5, -0.5)),
    ((9, 10), 1, (-2, 1), (0.125, -0.45)),
    ((9, 10), 1, (2, 2), (-0.5, -0.5)),
    # tiles of 16 x 64: the seam (row H - sy, column W - sx) at row 2 / column 98, strictly inside a tile ...
    ((72, 100), 4, (-2, 2), (0.3, 0.2)),
    # ... and at row 64 / column 64, on a tile edge in both directions (a roll beyond a prior's draws, legal for the entry)
    ((72, 100), 4, (8, 36), (-0.4, 0.15)),
]
# D = 256 (16 x 16 patches): (shape, stride, roll, offsets) on gmm16_cases.synthetic_mixture(K, SEED), the mixture
# tests/golden/gmm16.npz was generated with
CASES_256 = [((40, 44), 8, (4, -3), (0.3, -0.2)), ((40, 44), 8, (-4, 0), (-0.5, 0.5))]
GMM_META_STRIDE = image_norm_cases.GMM_META_STRIDE
FIXTURE_SEED = 2077  # generator seed of fixture case i: FIXTURE_SEED + i
FIT_SHAPE, FIT_EPOCHS, FIT_SEED = (32, 32), 6, 77


def case_flux(index, table=None):
    shape = (CASES if table is None else table)[index][0]
    return np.random.RandomState(4100 + index + (0 if table is None else 50)).gamma(20, size=shape).astype(np.float32)


def fixture_gmm(golden):
    """The K = 12 mixture of tests/golden/image_norm.npz (no new copy is stored)"""
    return image_norm_cases.fixture_gmm(golden)


def mixture256():
    return gmm16_cases.synthetic_mixture(gmm16_cases.K, gmm16_cases.SEED)


def staged(normed, roll, offsets):
    """s = conv2d(roll(normed), k, "same") of a (1, 1, H, W) tensor: the image the reference cuts its patches from.  The
    weights are the float32 numbers of `grid_weights` in every precision."""
    image = normed if roll is None else torch.roll(normed, shifts=tuple(int(s) for s in roll), dims=(normed.ndim - 2, normed.ndim - 1))
    kernel = prior_cases.subpix_kernel(*offsets).to(image.dtype).reshape(1, 1, 3, 3)
    return F.conv2d(image, kernel, padding="same")


def patch_log_like(image, gmm, stride, patch_norm="subtract-mean"):
    if patch_norm == "subtract-mean":
        return cpu_ref.gmm_patch_log_like(image, gmm, stride, None)
    assert patch_norm == "std-subtract-mean"
    return patch_norm_cases.patch_log_like(image, gmm, stride, None)[0]


def oracle(flux_np, norm, gmm_arrays, stride, roll, offsets, marginalize, dtype=np.float32, patch_norm="subtract-mean",
           meta_stride=GMM_META_STRIDE):
    """Sum over the patches of the per-patch value and its gradient with respect to the RAW flux (autograd), in `dtype`;
    max mode: also the arg-max per patch and the margin to the second-best component.  `norm`: a host image norm or None.
    The prior is `sum * stride^2 / D / numel`.  (No case has a filtered patch: the stencil of a positive image is >= 0.)"""
    with cpu_ref.precision(dtype):
        gmm = cpu_ref.GMM.from_numpy(*gmm_arrays, stride=meta_stride)
        flux = cpu_ref._tensor(flux_np[np.newaxis, np.newaxis]).requires_grad_(True)
        image = staged(flux if norm is None else norm(flux), roll, offsets)
        loglike = patch_log_like(image, gmm, stride, patch_norm)
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


_GMMS = {}


@functools.lru_cache(maxsize=None)
def _cached(index, marginalize, dtype_name, norm_type, patch_norm, table):
    cases = CASES if table == 64 else CASES_256
    shape, stride, roll, offsets = cases[index]
    norm = None if norm_type is None else image_norm_cases.make_norm(norm_type)
    arrays = _GMMS["fixture"] if table == 64 else mixture256()
    return oracle(case_flux(index, None if table == 64 else CASES_256), norm, arrays, stride, roll, offsets, marginalize,
                  np.dtype(dtype_name).type, patch_norm, GMM_META_STRIDE if table == 64 else gmm16_cases.STRIDE)


def cached_oracle(golden, index, marginalize, dtype, norm_type=None, patch_norm="subtract-mean", table=64):
    """`oracle` of CASES[index] (table 64) or CASES_256[index] (table 256), computed once per session and not changed"""
    _GMMS.setdefault("fixture", fixture_gmm(golden))
    return _cached(index, bool(marginalize), np.dtype(dtype).name, norm_type, patch_norm, table)


def near_border_or_seam(shape, roll):
    """Boolean (H, W) mask, un-rolled frame: pixels within one of a border of the rolled image -- the image border and the
    seam of the roll, where the zero padding acts"""
    H, W = shape
    sy, sx = (0, 0) if roll is None else roll
    Y = (np.arange(H) + sy) % H
    X = (np.arange(W) + sx) % W
    rows = (Y <= 1) | (Y >= H - 2)
    cols = (X <= 1) | (X >= W - 2)
    return rows[:, None] | cols[None, :]


def near_tie_mask(margin, shape, stride, roll, patch=8):
    """Pixels (un-rolled frame) a near-tie patch's gradient row can reach: the patch's cover, one pixel wider (the
    adjoint stencil), wrapped"""
    from conftest import patch_cover_mask

    ties = np.flatnonzero(np.asarray(margin) < NEAR_TIE)
    mask = patch_cover_mask(ties, shape, stride, roll, patch=patch)
    wide = mask.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            wide |= np.roll(mask, (dy, dx), axis=(0, 1))
    return wide


def draw(generator, patch_shape=(8, 8), cycle_spin=True):
    """One draw as the reference makes it: the two roll draws (rows first) when `cycle_spin`, then x0, then y0"""
    roll = cpu_ref.draw_cycle_spin_shifts(generator, patch_shape) if cycle_spin else None
    return roll, prior_cases.draw_offsets(generator)


class SubpixPatchPriorRef(cpu_ref.GMMPatchPriorRef):
    """`cpu_ref.GMMPatchPriorRef` with the sub-pixel cycle spin behind the roll: a callable for
    `cpu_ref.map_fit_sequential` with the reference's generator behaviour; `norm`: an image norm applied first."""

    def __init__(self, gmm, norm=None, **kwargs):
        super().__init__(gmm, **kwargs)
        self.norm = norm
        self.drawn = []

    def __call__(self, flux):
        roll, offsets = draw(self.generator, self.gmm.patch_shape, self.cycle_spin)
        self.last_shifts = (roll, offsets)
        self.drawn.append(self.last_shifts)
        image = staged(flux if self.norm is None else self.norm(flux), roll, offsets)
        return cpu_ref.gmm_patch_log_prior(image, self.gmm, self.stride, None, self.marginalize)


def rel_err(got, ref, keep=None):
    return image_norm_cases.rel_err(got, ref, keep)

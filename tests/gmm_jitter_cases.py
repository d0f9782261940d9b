"""Shared by tools/make_golden_gmm_jitter.py, tests/test_gmm_jitter_golden.py, tests/test_gmm_jitter_host.py (CPU) and
tests/test_gpu_gmm_jitter.py (GPU): the cases of the GMM patch prior with a jittered patch grid (`jitter=True`) and their
oracle.

The oracle restates the reference (jolideco/priors/patches/core.py:189-220, utils/torch.py:278-334) from torch and
`oracle/cpu_ref`: img = torch.roll(norm(flux)); the jittered patches laid side by side, S = img[..., R, :][..., C] with
R = (py[:, None] + arange(P)).ravel() and C likewise; the patch log-likelihoods of `cpu_ref` on S at stride P; max or
logsumexp, the sum, autograd.  It was pinned against the live reference when tools/make_golden_gmm_jitter.py generated
tests/golden/gmm_jitter.npz."""
import functools

import numpy as np
import torch

import image_norm_cases
import patch_norm_cases
from oracle import cpu_ref
from tools import gmm16_cases

NEAR_TIE = image_norm_cases.NEAR_TIE  # float64 margin between the two best components below which a patch is a near tie
TILE = (16, 64)  # rows x columns of a tile of the adjoint kernel (GJ_TY x GJ_TX of csrc/gmm_jitter.hip)

# (shape, stride, roll) on 8 x 8 patches; the draws of case i come from a generator seeded SEED + i (x first, then y).
# 0: a duplicate row and a duplicate column position | 1: non-monotonic positions | 2: 5 x 2 tiles of TILE | 3: overlap 2 |
# 4: odd height, W % 4 == 0 | 5: overlap 0 -- the draws are all 0 but are still drawn | 6: one patch row | 7: scalar paths,
# overlap 1.  Every shape is safe: max(base) + overlap <= n - P along both axes.
CASES = [
    ((40, 44), 4, (2, -1)),
    ((40, 44), 4, None),
    ((72, 100), 4, (-2, 2)),
    ((38, 42), 6, (1, 1)),
    ((41, 44), 5, (-1, 2)),
    ((24, 27), 8, (-2, -2)),
    ((16, 20), 4, (0, 0)),
    ((37, 41), 7, (2, 0)),
]
SEED = 3000
# D = 256 (16 x 16 patches) on gmm16_cases.synthetic_mixture(K, SEED), the mixture tests/golden/gmm16.npz was generated with
CASES_256 = [((48, 56), 8, (4, -3)), ((48, 50), 16, (-4, 0))]
SEED_256 = 3100
GMM_META_STRIDE = image_norm_cases.GMM_META_STRIDE
FIXTURE_SEED = 2177  # generator seed of fixture item i: FIXTURE_SEED + i
FIT_SHAPE, FIT_EPOCHS, FIT_SEED = (32, 32), 6, 78


def table_of(table):
    return (CASES, 8, SEED) if table == 64 else (CASES_256, 16, SEED_256)


def case_flux(index, table=64):
    (H, W), stride, _ = table_of(table)[0][index]
    return np.random.RandomState(5100 + H + W + stride).gamma(20, size=(H, W)).astype(np.float32)


def grid(shape, patch, stride):
    """(base_y, base_x) as numpy arrays: arange(overlap, n - stride - overlap, stride) per axis"""
    overlap = patch - stride
    return tuple(np.arange(overlap, n - stride - overlap, stride) for n in shape)


def is_safe(shape, patch, stride):
    overlap = patch - stride
    return all(len(b) > 0 and b[-1] + overlap <= n - patch for b, n in zip(grid(shape, patch, stride), shape))


def draw_jitter(generator, shape, patch, stride):
    """(jitter_y, jitter_x) as the reference draws them: `randint(-overlap, overlap + 1, (n_x,))` first, then the rows'"""
    base_y, base_x = grid(shape, patch, stride)
    overlap = patch - stride
    jitter_x = torch.randint(low=-overlap, high=overlap + 1, size=(len(base_x),), generator=generator)
    jitter_y = torch.randint(low=-overlap, high=overlap + 1, size=(len(base_y),), generator=generator)
    return jitter_y.numpy().astype(np.int64), jitter_x.numpy().astype(np.int64)


def draw(generator, shape, patch=8, stride=4, cycle_spin=True):
    """One draw as the reference makes it: the two roll draws (rows first) when `cycle_spin`, then the columns' jitter, then
    the rows': (roll or None, (jitter_y, jitter_x))"""
    roll = cpu_ref.draw_cycle_spin_shifts(generator, (patch, patch)) if cycle_spin else None
    return roll, draw_jitter(generator, shape, patch, stride)


def case_draws(index, table=64):
    """(jitter_y, jitter_x) of a case: from a generator seeded with the table's seed + index"""
    rows, patch, seed = table_of(table)
    shape, stride, _ = rows[index]
    return draw_jitter(torch.Generator("cpu").manual_seed(seed + index), shape, patch, stride)


def extreme_draws(shape=(40, 44), patch=8, stride=4):
    """Explicit draws on case 0's shape: all +overlap | all -overlap | alternating +overlap, -overlap (neighbouring rows swap
    places) | +overlap, 0 repeated (coincident neighbours)"""
    base_y, base_x = grid(shape, patch, stride)
    o = patch - stride
    out = {}
    for name, pattern in (("plus", (o,)), ("minus", (-o,)), ("alternating", (o, -o)), ("coincident", (o, 0))):
        out[name] = tuple(np.array([pattern[i % len(pattern)] for i in range(len(b))], dtype=np.int64) for b in (base_y, base_x))
    return out


def positions(shape, patch, stride, jitter):
    """(py, px): base + jitter per axis"""
    base_y, base_x = grid(shape, patch, stride)
    return base_y + np.asarray(jitter[0]), base_x + np.asarray(jitter[1])


def staged(normed, roll, py, px, patch):
    """S of a (1, 1, H, W) tensor: the jittered patches of the rolled image side by side"""
    image = normed if roll is None else torch.roll(normed, shifts=tuple(int(s) for s in roll), dims=(normed.ndim - 2, normed.ndim - 1))
    R = torch.from_numpy((np.asarray(py)[:, None] + np.arange(patch)).ravel().astype(np.int64))
    C = torch.from_numpy((np.asarray(px)[:, None] + np.arange(patch)).ravel().astype(np.int64))
    assert int(R.min()) >= 0 and int(R.max()) < image.shape[-2] and int(C.min()) >= 0 and int(C.max()) < image.shape[-1]
    return image[..., R, :][..., C]


def patch_log_like(image, gmm, patch, patch_norm="subtract-mean"):
    if patch_norm == "subtract-mean":
        return cpu_ref.gmm_patch_log_like(image, gmm, patch, None)
    assert patch_norm == "std-subtract-mean"
    return patch_norm_cases.patch_log_like(image, gmm, patch, None)[0]


def oracle(flux_np, norm, gmm_arrays, patch, stride, roll, jitter, marginalize, dtype=np.float32, patch_norm="subtract-mean",
           meta_stride=GMM_META_STRIDE):
    """Sum over the patches of the per-patch value and its gradient with respect to the RAW flux (autograd), in `dtype`;
    max mode: also the arg-max per patch (order i n_x + j) and the margin to the second-best component.  `norm`: a host
    image norm or None; `jitter` = (jitter_y, jitter_x).  The prior is `sum * stride^2 / P^2 / numel`."""
    py, px = positions(flux_np.shape, patch, stride, jitter)
    with cpu_ref.precision(dtype):
        gmm = cpu_ref.GMM.from_numpy(*gmm_arrays, stride=meta_stride)
        flux = cpu_ref._tensor(flux_np[np.newaxis, np.newaxis]).requires_grad_(True)
        image = staged(flux if norm is None else norm(flux), roll, py, px, patch)
        loglike = patch_log_like(image, gmm, patch, patch_norm)
        assert loglike.shape[0] == len(py) * len(px)  # (no case has a filtered patch)
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


def mixture256():
    return gmm16_cases.synthetic_mixture(gmm16_cases.K, gmm16_cases.SEED)


def fixture_gmm(golden):
    """The K = 12 mixture of tests/golden/image_norm.npz (no new copy is stored)"""
    return image_norm_cases.fixture_gmm(golden)


_GMMS = {}


@functools.lru_cache(maxsize=None)
def _cached(index, marginalize, dtype_name, norm_type, patch_norm, table, extreme):
    rows, patch, _ = table_of(table)
    shape, stride, roll = rows[index]
    jitter = case_draws(index, table) if extreme is None else extreme_draws(shape, patch, stride)[extreme]
    norm = None if norm_type is None else image_norm_cases.make_norm(norm_type)
    arrays = _GMMS["fixture"] if table == 64 else mixture256()
    return oracle(case_flux(index, table), norm, arrays, patch, stride, roll, jitter, marginalize, np.dtype(dtype_name).type,
                  patch_norm, GMM_META_STRIDE if table == 64 else gmm16_cases.STRIDE)


def cached_oracle(golden, index, marginalize, dtype, norm_type=None, patch_norm="subtract-mean", table=64, extreme=None):
    """`oracle` of a case (table 64 or 256; `extreme`: one of `extreme_draws` in place of the case's draws), computed once per
    session and not changed"""
    _GMMS.setdefault("fixture", fixture_gmm(golden))
    return _cached(index, bool(marginalize), np.dtype(dtype).name, norm_type, patch_norm, table, extreme)


def cover_lists(n, patch, stride, jitter, roll):
    """Brute force, per un-rolled pixel p of an axis of length n: the (i, a) pairs with pos_i + a == (p + roll) mod n, 0 <= a <
    patch, i ascending"""
    overlap = patch - stride
    pos = np.arange(overlap, n - stride - overlap, stride) + np.asarray(jitter)
    out = []
    for p in range(n):
        Y = (p + roll) % n
        out.append([(i, int(Y - pos[i])) for i in range(len(pos)) if 0 <= Y - pos[i] < patch])
    return out


def near_tie_mask(margin, shape, patch, stride, roll, jitter):
    """Pixels (un-rolled frame) a near-tie patch's gradient row reaches: its cover, from the jittered positions"""
    H, W = shape
    py, px = positions(shape, patch, stride, jitter)
    sy, sx = (0, 0) if roll is None else roll
    mask = np.zeros(shape, dtype=bool)
    for n in np.flatnonzero(np.asarray(margin) < NEAR_TIE):
        i, j = divmod(int(n), len(px))
        rows = (np.arange(py[i], py[i] + patch) - sy) % H
        cols = (np.arange(px[j], px[j] + patch) - sx) % W
        mask[np.ix_(rows, cols)] = True
    return mask


def covered_mask(shape, patch, stride, roll, jitter):
    """Pixels (un-rolled frame) at least one patch covers"""
    sy, sx = (0, 0) if roll is None else roll
    rows = np.array([bool(c) for c in cover_lists(shape[0], patch, stride, jitter[0], sy)])
    cols = np.array([bool(c) for c in cover_lists(shape[1], patch, stride, jitter[1], sx)])
    return rows[:, None] & cols[None, :]


class JitterPatchPriorRef(cpu_ref.GMMPatchPriorRef):
    """`cpu_ref.GMMPatchPriorRef` with the jittered grid behind the roll: a callable for `cpu_ref.map_fit_sequential` with
    the reference's generator behaviour; `norm`: an image norm applied first."""

    def __init__(self, gmm, norm=None, **kwargs):
        super().__init__(gmm, **kwargs)
        self.norm = norm
        self.drawn = []

    def __call__(self, flux):
        patch = self.gmm.patch_shape[0]
        roll, jitter = draw(self.generator, tuple(flux.shape[-2:]), patch, self.stride, self.cycle_spin)
        self.last_shifts = (roll, jitter)
        self.drawn.append(self.last_shifts)
        py, px = positions(tuple(flux.shape[-2:]), patch, self.stride, jitter)
        image = staged(flux if self.norm is None else self.norm(flux), roll, py, px, patch)
        loglike = cpu_ref.gmm_patch_log_like(image, self.gmm, patch, None)
        values = torch.logsumexp(loglike, dim=1) if self.marginalize else torch.max(loglike, dim=1).values
        return torch.sum(values) * (self.stride**2 / patch**2) / flux.numel()


def rel_err(got, ref, keep=None):
    return image_norm_cases.rel_err(got, ref, keep)

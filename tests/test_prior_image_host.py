"""CPU: the host side of `GMMPatchPrior.prior_image` / `prior_image_average` -- `GaussianMixtureModel.eigen_images`,
`reduce_to_topk`, `is_equal`, the restatement the GPU tests compare with (tests/prior_image_cases.py) and the refusals,
which are raised before the generator advances and before anything touches a device."""
import numpy as np
import pytest
import torch

import prior_image_cases as cases
from jolideco_amd.utils.norms import IdentityImageNorm


def _model(arrays, stride):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


@pytest.fixture(scope="module")
def model(golden):
    *arrays, stride = cases.mixture(golden, 8)
    return _model(arrays, stride)


# ------------------------------------------------------------------------------------------------ 1. the mixture's new surface
@pytest.mark.parametrize("patch", [8, 16])
def test_eigen_images(golden, patch):
    *arrays, stride = cases.mixture(golden, patch)
    gmm = _model(arrays, stride)
    images = gmm.eigen_images
    assert images.shape == (gmm.n_components, patch, patch) and images.dtype == np.float64 and np.isfinite(images).all()
    assert gmm.eigen_images is images  # cached
    # sum_j w_j v_j has the squared norm sum_j w_j^2 = |cov|_F^2 whatever the signs of the eigenvectors
    cov = gmm.covariances_numpy.astype(np.float64)
    for k in range(gmm.n_components):
        assert np.linalg.norm(images[k]) == pytest.approx(np.linalg.norm(cov[k]), rel=1e-10)


def test_reduce_to_topk(model):
    top = model.reduce_to_topk(5)
    order = np.argsort(model.weights_numpy)[::-1][:5]
    assert top.n_components == 5 and np.all(np.diff(top.weights_numpy) <= 0)
    assert np.array_equal(top.weights_numpy, model.weights_numpy[order])
    assert np.array_equal(top.means_numpy, model.means_numpy[order])
    assert np.array_equal(top.covariances_numpy, model.covariances_numpy[order])
    assert top.meta is model.meta and top.meta.stride == cases.GMM_META_STRIDE


def test_is_equal(golden, model):
    *arrays, stride = cases.mixture(golden, 8)
    assert model.is_equal(_model(arrays, stride))
    assert not model.is_equal(model.reduce_to_topk(5))  # another shape
    means, covariances, weights = arrays
    assert not model.is_equal(_model((means, covariances * 1.01, weights), stride))  # other covariances


# ------------------------------------------------------------------------------------------------ 2. the restatement
@pytest.mark.parametrize("shape", [(40, 44), (43, 50)])
def test_restatement_of_a_constant(golden, shape):
    """A zero table and the identity norm reconstruct constant x (sum of the covering patches' weights): the constant where
    that sum is 1 -- at least `overlap` from every border of the covered region --, strictly less on its border, and 0
    on rows and columns no patch reaches ((43, 50) at stride 4: rows 40 .. 42, columns 48, 49)."""
    stride, patch, constant = 4, 8, 7.25
    *arrays, meta_stride = cases.mixture(golden, patch)
    table = np.zeros((arrays[0].shape[0], patch, patch))
    image, _, _ = cases.restated(np.full(shape, constant, dtype=np.float32), IdentityImageNorm(), tuple(arrays), stride, None,
                                 table, np.float64, meta_stride)
    n_y, n_x = cases.n_patches(shape, stride, patch)
    bottom, right = (n_y - 1) * stride + patch, (n_x - 1) * stride + patch  # the covered region
    overlap = patch - stride
    interior = image[overlap : bottom - overlap, overlap : right - overlap]
    assert interior.size and np.allclose(interior, constant, rtol=1e-6, atol=0)
    assert np.allclose(cases.weight_sum(shape, stride, patch)[overlap : bottom - overlap, overlap : right - overlap], 1.0, rtol=1e-12)
    for border in (image[0, :right], image[bottom - 1, :right], image[:bottom, 0], image[:bottom, right - 1]):
        assert (border > 0).all() and (border < constant).all()
    assert (image[bottom:] == 0).all() and (image[:, right:] == 0).all()
    if shape == (43, 50):
        assert bottom == 40 and right == 48


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_cases_are_finite_and_have_few_near_ties(golden, name):
    """What the GPU file relies on: the float64 restatement of every case is finite (under a norm: the table is scaled so
    that R stays inside the inverse's domain), no patch is filtered, and at most 1 % of the patches are near ties."""
    image, arg, margin = cases.cached_restated(golden, name, np.float64)
    patch, shape, stride, roll, _ = cases.CASES[name]
    n_y, n_x = cases.n_patches(shape, stride, patch)
    assert image.shape == shape and np.isfinite(image).all() and np.abs(image).max() > 0
    assert arg.shape == margin.shape == (n_y * n_x,) and (margin >= 0).all()
    keep, clear = cases.kept_pixels(margin, name)
    assert (~clear).sum() <= 0.01 * clear.size, f"{(~clear).sum()} near ties among {clear.size} patches"
    assert keep.any()
    if cases.CASES[name][4] is None:  # (normed patches are small: one component may win them all)
        assert len(np.unique(arg)) > 1, "one winner everywhere: the table's gather is not exercised"


def test_the_tile_case_spans_ragged_tiles():
    shape = cases.CASES["tiles"][1]
    for n, t in zip(shape, cases.TILE):
        assert n > 2 * t and n % t != 0


# ------------------------------------------------------------------------------------------------ 3. refusals
def _state(generator):
    return generator.get_state().clone()


def _refused(prior, error, match=None, **kwargs):
    flux = np.full((40, 44), 20.0, dtype=np.float32)
    for method in (prior.prior_image, prior.prior_image_average):
        before = _state(prior.generator)
        with pytest.raises(error, match=match):
            method(flux, **kwargs)
        assert torch.equal(_state(prior.generator), before), "the generator advanced"


def test_refusals_leave_the_generator_alone(model):
    from jolideco_amd.priors.patches.core import GMMPatchPrior, JitteredGMMPatchPrior, MultiScalePrior, SubpixelGMMPatchPrior
    from jolideco_amd.utils.norms import StandardizedSubtractMeanPatchNorm

    gen = lambda: torch.Generator().manual_seed(5)  # noqa: E731
    _refused(JitteredGMMPatchPrior(gmm=model, stride=4, generator=gen()), ValueError,
             match="Computing prior images with jittering is not supported.")
    _refused(SubpixelGMMPatchPrior(gmm=model, stride=4, generator=gen()), NotImplementedError, match="cycle_spin_subpix")
    _refused(GMMPatchPrior(gmm=model, stride=4, generator=gen(), patch_norm=StandardizedSubtractMeanPatchNorm()),
             NotImplementedError, match="std-subtract-mean")
    _refused(GMMPatchPrior(gmm=model, stride=8, generator=gen()), ValueError, match="stride 8")
    plain = GMMPatchPrior(gmm=model, stride=4, generator=gen())
    _refused(plain, ValueError, match="patch_images must have shape", patch_images=np.zeros((model.n_components, 8, 7)))
    _refused(plain, ValueError, match="patch_images must have shape", patch_images=np.zeros((model.n_components + 1, 8, 8)))
    before = _state(plain.generator)
    with pytest.raises(ValueError, match="n_average"):
        plain.prior_image_average(np.full((40, 44), 20.0, dtype=np.float32), n_average=0)
    assert torch.equal(_state(plain.generator), before)
    assert not hasattr(MultiScalePrior, "prior_image") and not hasattr(MultiScalePrior, "prior_image_average")


def test_c_entry_is_declared_and_bound():
    import re
    from pathlib import Path

    from jolideco_amd import _hip

    repo = Path(__file__).resolve().parents[1]
    header = re.sub(r"/\*.*?\*/", "", (repo / "include" / "jolideco_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint jd_gmm_prior_image\s*\(jd_gmm\* gmm, const float\* flux, int H, int W, int stride,", header)
    assert "jd_gmm_prior_image" in _hip.EXPORTS and len(_hip.EXPORTS["jd_gmm_prior_image"][1]) == 13
    assert "gmm_prior_image.hip" in (repo / "jolideco_amd" / "csrc" / "Makefile").read_text()
    source = (repo / "jolideco_amd" / "csrc" / "gmm_prior_image.hip").read_text()
    tile = re.search(r"PI_TX = (\d+), PI_TY = (\d+)", source)
    assert tile and (int(tile.group(2)), int(tile.group(1))) == cases.TILE

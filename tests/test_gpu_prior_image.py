"""GPU: `GMMPatchPrior.prior_image` / `prior_image_average` (csrc/gmm_prior_image.hip, jd_gmm_prior_image): the unchanged
max-mode forward pass, then the patch means and the overlap-add of a (K, P, P) table through the inverse image norm.

Yardstick: the float64 restatement of tests/prior_image_cases.py.  The error is max|got - ref| / max|ref| over the kept
pixels and must be <= max(1e-5, 4 e_ref), e_ref the float32 restatement's own error against the float64 one (the bound
form of tests/test_gpu_gmm_subpix.py; 1e-5 is the project's image tolerance).  A patch whose float64 margin between its
two best components is below NEAR_TIE may resolve differently in float32: the pixels it covers are left out (at most 1 % of
a case's patches, asserted on the restatement in tests/test_prior_image_host.py).
"""
import numpy as np
import pytest
import torch

import prior_image_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(golden, patch):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    *arrays, stride = cases.mixture(golden, patch)
    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


@pytest.fixture(scope="module")
def models(golden):
    return {8: _model(golden, 8), 16: _model(golden, 16)}


def _dev(array):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(DEV)


def _image(model, flux_np, stride, roll, table, norm=None, out=None, scale=1.0, accumulate=False):
    """One low-level call with a given roll: the image as float32 numpy"""
    handle = model.handle(DEV)
    out = torch.full(flux_np.shape, np.nan, dtype=torch.float32, device=DEV) if out is None else out
    handle.prior_image(_dev(flux_np), stride, roll, handle.prior_image_table(table), out, scale=scale, accumulate=accumulate,
                       norm=norm)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _prior(model, stride=4, seed=11, **kwargs):
    from jolideco_amd.priors.patches.core import GMMPatchPrior

    return GMMPatchPrior(gmm=model, stride=stride, generator=torch.Generator().manual_seed(seed), device=DEV, **kwargs)


def _check_parity(label, got, ref64, ref32, keep):
    scale = np.abs(ref64).max()
    err = float(np.abs(got - ref64)[keep].max() / scale)
    e_ref = float(np.abs(ref32 - ref64)[keep].max() / scale)
    print(f"prior image parity {label}: e_ref {e_ref:.2e} device {err:.2e} ({int((~keep).sum())} pixels of near-tie patches left out)")
    assert np.isfinite(got).all()
    assert err <= max(1e-5, 4 * e_ref)


# ------------------------------------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_image_matches_the_restatement(golden, models, name):
    patch, shape, stride, roll, _ = cases.CASES[name]
    ref64, _, margin = cases.cached_restated(golden, name, np.float64)
    ref32, _, _ = cases.cached_restated(golden, name, np.float32)
    keep, _ = cases.kept_pixels(margin, name)
    model = models[patch]
    got = _image(model, cases.case_flux(name), stride, roll, cases.case_table(name, model.n_components), cases.case_norm(name))
    _check_parity(name, got, ref64, ref32, keep)


def test_scale_and_accumulate(golden, models):
    """out += scale * image: the form `prior_image_average` is built from"""
    name = "s4-roll-a"
    patch, shape, stride, roll, _ = cases.CASES[name]
    model = models[patch]
    flux, table = cases.case_flux(name), cases.case_table(name, model.n_components)
    plain = _image(model, flux, stride, roll, table)
    base = np.random.RandomState(3).normal(size=shape).astype(np.float32)
    got = _image(model, flux, stride, roll, table, out=_dev(base), scale=0.25, accumulate=True)
    assert np.array_equal(got, base + np.float32(0.25) * plain)
    assert np.array_equal(_image(model, flux, stride, roll, table, out=_dev(base), scale=0.25), np.float32(0.25) * plain)


@pytest.mark.parametrize("roll", [None, (2, -1)])
def test_zero_table_and_constant_flux(models, roll):
    """Identity norm: constant x (sum of the covering patches' weights) -- the constant in the interior, exactly 0 on the
    rows and columns no patch reaches ((43, 50) at stride 4: 3 rows and 2 columns of the rolled frame)"""
    shape, stride, patch, constant = (43, 50), 4, 8, 7.25
    model = models[patch]
    got = _image(model, np.full(shape, constant, dtype=np.float32), stride, roll, np.zeros((model.n_components, patch, patch)))
    weights = cases.weight_sum(shape, stride, patch)
    if roll is not None:
        weights = np.roll(weights, shift=(-roll[0], -roll[1]), axis=(0, 1))
    interior, uncovered = np.isclose(weights, 1.0, rtol=1e-12), weights == 0
    assert interior.sum() == (40 - 8) * (48 - 8) and uncovered.sum() == 43 * 50 - 40 * 48
    assert np.abs(got[interior] - constant).max() <= 1e-6 * constant
    assert (got[uncovered] == 0).all()
    assert np.abs(got - constant * weights).max() <= 1e-6 * constant


# ------------------------------------------------------------------------------------------------ 2. the methods
def test_default_table_is_the_eigen_images(golden, models):
    """`prior_image` without a table against the restatement with `gmm.eigen_images` (the same array on both sides: the
    eigenvectors' signs do not enter), for the roll the prior drew"""
    name = "s4-roll-a"
    patch, shape, stride, _, _ = cases.CASES[name]
    model, flux = models[patch], cases.case_flux(name)
    prior = _prior(model, stride)
    got = prior.prior_image(flux)
    roll = prior.last_shifts
    assert got.dtype == np.float32 and got.shape == shape and roll is not None
    *arrays, meta_stride = cases.mixture(golden, patch)
    results = [cases.restated(flux, prior.norm, tuple(arrays), stride, roll, model.eigen_images, dtype, meta_stride)
               for dtype in (np.float64, np.float32)]
    clear = results[0][2] >= cases.NEAR_TIE
    assert (~clear).sum() <= 0.01 * clear.size
    from conftest import patch_cover_mask

    keep = ~patch_cover_mask(np.flatnonzero(~clear), shape, stride, roll, patch=patch)
    _check_parity("eigen-images", got, results[0][0], results[1][0], keep)


def test_patch_images_override_the_default_table(models):
    name = "s4-roll-a"
    patch, shape, stride, _, _ = cases.CASES[name]
    model, flux = models[patch], cases.case_flux(name)
    table = cases.case_table(name, model.n_components)
    default = _prior(model, stride).prior_image(flux)
    prior = _prior(model, stride)
    got = prior.prior_image(flux, patch_images=table)
    assert np.array_equal(got, _image(model, flux, stride, prior.last_shifts, table))
    assert np.abs(got - default).max() > 0
    assert np.array_equal(_prior(model, stride).prior_image(flux), default)  # (the handle's cached table was replaced)


def test_marginalize_and_reruns_give_the_same_bits(models):
    name = "s2"
    patch, shape, stride, _, _ = cases.CASES[name]
    model, flux = models[patch], cases.case_flux(name)
    first = _prior(model, stride).prior_image_average(flux, n_average=2)
    again = _prior(model, stride).prior_image_average(flux, n_average=2)
    marginal = _prior(model, stride, marginalize=True).prior_image_average(flux, n_average=2)
    assert np.array_equal(first, again) and np.array_equal(first, marginal)


def test_average_is_the_mean_of_the_draws(models):
    name = "s4-roll-a"
    patch, shape, stride, _, _ = cases.CASES[name]
    model, flux = models[patch], cases.case_flux(name)
    average = _prior(model, stride, seed=23).prior_image_average(flux, n_average=3)
    prior = _prior(model, stride, seed=23)
    draws, rolls = [], []
    for _ in range(3):
        draws.append(prior.prior_image(flux).astype(np.float64))
        rolls.append(prior.last_shifts)
    assert len(set(rolls)) > 1  # (the draws differ: the mean is not that of one image)
    mean = np.mean(draws, axis=0)
    assert np.abs(average - mean).max() <= 1e-6 * np.abs(mean).max()


def test_generator_advances_as_for_one_evaluation(models):
    model, flux = models[8], cases.case_flux("s4-roll-a")
    prior, twin = _prior(model, seed=31), _prior(model, seed=31)
    prior.prior_image(flux)
    shifts = twin.draw_shifts(flux.shape)
    assert prior.last_shifts == shifts
    assert torch.equal(prior.generator.get_state(), twin.generator.get_state())
    off, off_twin = _prior(model, seed=31, cycle_spin=False), _prior(model, seed=31, cycle_spin=False)
    off.prior_image(flux)
    assert off.last_shifts is None and torch.equal(off.generator.get_state(), off_twin.generator.get_state())


def test_numpy_and_tensor_inputs_agree(models):
    model, flux = models[8], cases.case_flux("s4-roll-a")
    from_numpy = _prior(model).prior_image(flux)
    assert np.array_equal(_prior(model).prior_image(_dev(flux)), from_numpy)
    assert np.array_equal(_prior(model).prior_image(_dev(flux)[None, None]), from_numpy)


# ------------------------------------------------------------------------------------------------ 3. the C entry's refusals
@pytest.mark.parametrize("patch", [8, 16])
def test_invalid_arguments_launch_nothing(models, patch):
    from jolideco_amd import _hip
    from jolideco_amd.ops import ptr, stream_ptr
    from jolideco_amd.utils.norms import StandardizedSubtractMeanPatchNorm

    name = "s4-roll-a" if patch == 8 else "p16-roll-a"
    _, shape, stride, roll, _ = cases.CASES[name]
    model = models[patch]
    handle, lib = model.handle(DEV), _hip.lib()
    flux_np, table_np = cases.case_flux(name), cases.case_table(name, model.n_components)
    before = _image(model, flux_np, stride, roll, table_np)
    flux, table = _dev(flux_np), handle.prior_image_table(table_np)

    def prior_value():
        value = torch.full((1,), np.nan, device=DEV)
        handle.prior_fwd_bwd(flux, stride, roll, value, 1.0)
        return float(value)

    value_before = prior_value()
    sentinel = np.float32(-12345.0)
    out = torch.full(shape, float(sentinel), dtype=torch.float32, device=DEV)
    H, W = shape

    def call(h=handle._handle, f=flux, t=table, o=out, height=H, width=W, s=stride):
        return lib.jd_gmm_prior_image(h, ptr(f), height, width, s, 0, 0, ptr(t), 1.0, ptr(o), 0, None, stream_ptr(flux.device))

    handle.set_image_norm(None), handle.set_patch_norm(None)
    for kwargs in ({"h": None}, {"f": None}, {"t": None}, {"o": None}):
        assert call(**kwargs) == -1 and b"jd_gmm_prior_image: null argument" in lib.jd_last_error()
    assert call(height=patch - 1) == -1 and call(width=patch - 1) == -1 and b"smaller than a patch" in lib.jd_last_error()
    assert call(s=0) == -1 and call(s=patch) == -1 and b"stride" in lib.jd_last_error()
    handle.set_patch_norm(StandardizedSubtractMeanPatchNorm())
    assert call() == -1 and b"standardized" in lib.jd_last_error()
    handle.set_patch_norm(None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == sentinel).all()  # nothing was launched
    assert np.isfinite(value_before) and prior_value() == value_before  # the handle evaluates the prior as before
    assert np.array_equal(_image(model, flux_np, stride, roll, table_np), before)

"""CPU: the standardized patch norm of the GMM patch prior, x = (p - mean(p)) / mean(p) ("std-subtract-mean"), against
tests/golden/patch_norm.npz, generated from the LIVE reference by tools/make_golden_patch_norm.py: host class,
(de)serialisation, mixture files, construction, the oracle of the GPU tests (tests/patch_norm_cases.py), the inputs of
those tests (near ties, responsibilities) and the refusals."""
import json

import numpy as np
import pytest
import torch

import patch_norm_cases as cases
from conftest import rel_linf
from image_norm_cases import SHAPE_CASES, case_flux, fixture_gmm
from tools import gmm16_cases

from jolideco_amd import GMMPatchPrior, SpatialFluxComponent
from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
from jolideco_amd.utils import norms
from jolideco_amd.utils.io._fitsfile import read_fits

NAME = "std-subtract-mean"


def test_patch_norm_registry_and_dict_round_trip():
    """Fails on the commit before the norm: `PatchNorm.from_dict` raised NotImplementedError for this type."""
    norm = norms.PatchNorm.from_dict({"type": NAME})
    assert type(norm) is norms.StandardizedSubtractMeanPatchNorm and "StandardizedSubtractMeanPatchNorm" in norms.__all__
    assert norm.to_dict() == {"type": NAME}
    assert type(norms.PatchNorm.from_dict(norm.to_dict())) is type(norm)
    assert sorted(norms.NORMS_PATCH_REGISTRY) == [NAME, "subtract-mean"]
    assert norms.SubtractMeanPatchNorm().to_dict() == {"type": "subtract-mean"}
    assert (norms.SubtractMeanPatchNorm.device_kind, norms.StandardizedSubtractMeanPatchNorm.device_kind) == (0, 1)
    with pytest.raises(NotImplementedError):
        norms.PatchNorm.from_dict({"type": "divide-by-max"})


def test_host_call_is_the_formula():
    x = torch.from_numpy(np.random.RandomState(3).gamma(20, size=(9, 64)).astype(np.float32))
    got = norms.StandardizedSubtractMeanPatchNorm()(x)
    mean = x.mean(dim=1, keepdim=True)
    assert got.dtype == torch.float32 and torch.equal(got, (x - mean) / mean)
    assert torch.equal(got, cases.standardize(x))
    assert float(got.mean(dim=1).abs().max()) < 1e-6  # (relative contrast: mean free)
    scaled = norms.StandardizedSubtractMeanPatchNorm()(4.0 * x)
    assert torch.equal(scaled, got)  # scale invariant (a power of two: exactly)


def _standardized_gmm(golden, **meta):
    meta = GaussianMixtureModelMeta(stride=4, patch_norm=norms.StandardizedSubtractMeanPatchNorm(), **meta)
    return GaussianMixtureModel.from_numpy(*fixture_gmm(golden), meta=meta)


@pytest.fixture()
def gmm_library(tmp_path, monkeypatch, golden):
    """A user's GMM library directory with the fixture's mixture, trained on standardized patches, registered as
    "zoran-weiss" (the pattern of tests/test_image_norm_golden.py)."""
    gmm = _standardized_gmm(golden)
    gmm.write(tmp_path / "zw.fits")
    index = {"zoran-weiss": {"filename": "$JOLIDECO_GMM_LIBRARY/zw.fits", "format": "table"}}
    (tmp_path / "jolideco-gmm-library-index.json").write_text(json.dumps(index))
    monkeypatch.setenv("JOLIDECO_GMM_LIBRARY", str(tmp_path))
    return gmm


def test_table_file_carries_the_patch_norm(golden, tmp_path):
    """A mixture written with the norm names it in PNPTYPE; read back as a table it carries it, and a prior built on it
    takes it."""
    gmm = _standardized_gmm(golden)
    gmm.write(tmp_path / "std.fits")
    new = GaussianMixtureModel.read(tmp_path / "std.fits", format="table")
    assert type(new.meta.patch_norm) is norms.StandardizedSubtractMeanPatchNorm
    prior = GMMPatchPrior(gmm=new)
    assert type(prior.patch_norm) is norms.StandardizedSubtractMeanPatchNorm
    assert prior.to_dict()["patch_norm"] == {"type": NAME}
    # an explicit norm wins over the mixture's, both ways
    assert type(GMMPatchPrior(gmm=new, patch_norm=norms.SubtractMeanPatchNorm()).patch_norm) is norms.SubtractMeanPatchNorm
    plain = GaussianMixtureModel.from_numpy(*fixture_gmm(golden), meta=GaussianMixtureModelMeta(stride=4))
    assert type(GMMPatchPrior(gmm=plain).patch_norm) is norms.SubtractMeanPatchNorm
    both = GMMPatchPrior(gmm=plain, patch_norm=norms.StandardizedSubtractMeanPatchNorm())
    assert both.to_dict()["patch_norm"] == {"type": NAME}
    assert (both.supports_fused_step, both.supports_phases, both.shardable) == (True, True, True)

    class OtherNorm(norms.PatchNorm):  # a norm without a device kernel is refused, never run some other way
        pass

    with pytest.raises(NotImplementedError, match="OtherNorm"):
        GMMPatchPrior(gmm=plain, patch_norm=OtherNorm())


@pytest.mark.parametrize("format", ["fits", "yaml"])
def test_component_with_a_standardized_prior_round_trips(format, tmp_path, gmm_library):
    prior = GMMPatchPrior()
    assert type(prior.patch_norm) is norms.StandardizedSubtractMeanPatchNorm
    assert type(GMMPatchPrior.from_dict(prior.to_dict()).patch_norm) is norms.StandardizedSubtractMeanPatchNorm
    component = SpatialFluxComponent(flux_upsampled=torch.ones((1, 1, 16, 16)), prior=prior)
    filename = tmp_path / f"component.{format}"
    component.write(filename=filename, format=format)
    new = SpatialFluxComponent.read(filename=filename, format=format)
    assert type(new.prior.patch_norm) is norms.StandardizedSubtractMeanPatchNorm
    assert new.prior.to_dict()["patch_norm"] == {"type": NAME}
    if format == "fits":
        assert read_fits(filename)[0].header["PNPTYPE"] == NAME
    else:
        text = filename.read_text()
        assert f"type: {NAME}" in text and "!!python" not in text


# ------------------------------------------------------------------------------------------------ oracle and fixture
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("normed", [False, True])
@pytest.mark.parametrize("d", [64, 256])
def test_oracle_reproduces_the_reference_prior(golden, d, normed, marginalize):
    """tests/patch_norm_cases.oracle = the reference's GMMPatchPrior(patch_norm=StandardizedSubtractMeanPatchNorm(),
    cycle_spin=False): value at rel 1e-5, gradient at relative L-infinity 1e-5 (bit for bit when the fixture was
    generated)."""
    g = golden("patch_norm")
    norm = cases.asinh_norm() if normed else None
    assert norm is None or (float(norm.alpha), float(norm.beta)) == tuple(float(v) for v in g["asinh/params"])
    if d == 64:
        flux, arrays, stride, meta_stride = case_flux(0), fixture_gmm(golden), 4, 4
    else:
        arrays = gmm16_cases.synthetic_mixture(gmm16_cases.K, gmm16_cases.SEED)
        assert gmm16_cases.mixture_checksum(arrays) == pytest.approx(float(g["d256/gmm/checksum"]), rel=1e-13)
        flux, stride, meta_stride = gmm16_cases.fixture_flux(filtered=False), gmm16_cases.STRIDE, gmm16_cases.STRIDE
    o = cases.oracle(flux, arrays, stride, None, marginalize, norm=norm, meta_stride=meta_stride)
    scale = stride**2 / d / flux.size
    tag = f"d{d}/{'asinh' if normed else 'bare'}/{'lse' if marginalize else 'max'}"
    assert g[f"{tag}/value"].dtype == np.float32 and g[f"{tag}/grad"].dtype == np.float32
    assert o["total"] * scale == pytest.approx(float(g[f"{tag}/value"]), rel=1e-5)
    assert rel_linf(o["grad"] * scale, g[f"{tag}/grad"]) < 1e-5
    assert np.abs(g[f"{tag}/grad"]).max() > 0 and o["keep"].all()


def _max_mode_inputs(golden):
    """(label, float64 oracle) of every max-mode parity input of tests/test_gpu_patch_norm.py"""
    for index in range(len(SHAPE_CASES)):
        for normed in (False, True):
            yield f"d64 {SHAPE_CASES[index]} {'asinh' if normed else 'identity'}", cases.cached_oracle64(golden, index, False, normed, np.float64)
    for index in range(len(cases.SHAPES_256)):
        for shifts in cases.SHIFTS_256:
            yield f"d256 {cases.SHAPES_256[index]} {shifts}", cases.cached_oracle256(index, shifts, False, "float64")


def test_near_ties_of_the_gpu_cases_stay_within_one_percent(golden):
    """The GPU parity tests may leave patches whose two best float64 log-likelihoods differ by less than 1e-3 out of the
    arg-max and gradient comparison: at most 1 % of the patches of every input, on the oracle alone.  Measured when the
    tests were written: no such patch in any input (smallest D = 64 margin 0.034); the smallest D = 256 margin is 52.7."""
    smallest256 = np.inf
    for label, o in _max_mode_inputs(golden):
        near = int((o["margin"] < cases.NEAR_TIE).sum())
        print(f"near ties {label}: {near} of {o['margin'].size}, smallest margin {o['margin'].min():.3g}")
        assert near <= 0.01 * o["margin"].size, (label, near, o["margin"].size)
        assert o["arg"].size == o["margin"].size > 0 and o["keep"].all()
        if label.startswith("d256"):
            smallest256 = min(smallest256, float(o["margin"].min()))
    assert smallest256 >= 40.0


def test_logsumexp_cases_exercise_the_responsibilities(golden):
    """At least one logsumexp input differs from its max sum by more than 1e-3 relative: more than one component carries
    weight, so the backward pass really sums over k."""
    gaps = []
    for index in range(len(SHAPE_CASES)):
        lse = cases.cached_oracle64(golden, index, True, False, np.float64)["total"]
        top = cases.cached_oracle64(golden, index, False, False, np.float64)["total"]
        gaps.append(abs(lse - top) / abs(top))
        print(f"logsumexp against max {SHAPE_CASES[index]}: {lse:.6g} against {top:.6g}")
    assert max(gaps) > 1e-3


# ------------------------------------------------------------------------------------------------ refusals
def test_compute_error_with_the_standardized_norm_raises_when_the_session_is_created(golden):
    """`hessian_ones` returns zeros because a constant is in the null space of a mean-subtracted patch; not so under the
    standardized norm.  The refusal names the patch norm, and comes before anything touches a device."""
    import jolideco_amd as jd
    from jolideco_amd.core import FitSession
    from jolideco_amd.data import point_source_gauss_psf
    from jolideco_amd.distributed import DistContext

    rs = np.random.RandomState(1)
    datasets = {"o": point_source_gauss_psf(shape=(32, 32), sigma_psf=2, random_state=rs)}
    datasets["o"].pop("flux")
    prior = GMMPatchPrior(gmm=_standardized_gmm(golden))
    comps = jd.FluxComponents()
    comps["flux"] = SpatialFluxComponent.from_numpy(flux=rs.gamma(30, size=(32, 32)), prior=prior)
    deco = jd.MAPDeconvolver(n_epochs=1, device="cuda:0", compute_error=True)
    with pytest.raises(NotImplementedError, match="compute_error=True .* patch norm 'std-subtract-mean'"):
        FitSession(deco, datasets, None, comps, DistContext.current())
    with pytest.raises(NotImplementedError, match="std-subtract-mean"):
        prior.hessian_ones(torch.ones((1, 1, 32, 32)))
    plain = GMMPatchPrior(gmm=GaussianMixtureModel.from_numpy(*fixture_gmm(golden), meta=GaussianMixtureModelMeta(stride=4)))
    assert not plain.hessian_ones(torch.ones((1, 1, 32, 32))).any()


def test_jitter_and_subpixel_cycle_spin_still_raise(golden):
    gmm = _standardized_gmm(golden)
    with pytest.raises(NotImplementedError, match="jitter"):
        GMMPatchPrior(gmm=gmm, jitter=True)
    with pytest.raises(NotImplementedError, match="cycle_spin_subpix"):
        GMMPatchPrior(gmm=gmm, cycle_spin_subpix=True)


def test_c_abi_of_the_patch_norm():
    """The new symbol is exported and bound; an unknown kind or a null handle returns JD_ERR_INVALID with a message."""
    from jolideco_amd import _hip

    lib = _hip.lib()
    assert "jd_gmm_set_patch_norm" in _hip.EXPORTS and hasattr(lib, "jd_gmm_set_patch_norm")
    for kind in (2, -1):
        assert lib.jd_gmm_set_patch_norm(None, kind) == -1
        assert b"unknown patch norm kind" in lib.jd_last_error()
    for kind in (0, 1):
        assert lib.jd_gmm_set_patch_norm(None, kind) == -1 and b"null argument" in lib.jd_last_error()
    assert "jd_gmm_set_const_residual" in _hip.EXPORTS and hasattr(lib, "jd_gmm_set_const_residual")
    assert lib.jd_gmm_set_const_residual(None, None) == -1 and b"null argument" in lib.jd_last_error()


@pytest.mark.parametrize("d", [64, 256])
def test_float64_constants_of_a_mixture(golden, d):
    """`const_float64_numpy`: the float64 oracle's constants to 1e-6 absolute (the factors are float32 numbers), where
    the float32 sum the library gets as const_k is off by up to a few 1e-5 -- the residual the standardized passes add."""
    from oracle import cpu_ref

    arrays = fixture_gmm(golden) if d == 64 else gmm16_cases.synthetic_mixture(gmm16_cases.K, gmm16_cases.SEED)
    gmm = GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=4 if d == 64 else 8))
    with cpu_ref.precision(np.float64):
        ref = cpu_ref.GMM.from_numpy(*arrays, stride=4 if d == 64 else 8)
        exact = -0.5 * d * np.log(2 * np.pi) + ref.log_det_cholesky.numpy() + ref.log_weights.numpy()
    got = gmm.const_float64_numpy
    assert got.dtype == np.float64 and got.shape == (len(arrays[2]),)
    assert np.abs(got - exact).max() < 1e-6
    const32 = (np.float32(-0.5) * (np.float32(d) * np.float32(np.log(np.float32(2 * np.pi)))) + gmm.log_det_cholesky_numpy
               + gmm.log_weights_numpy).astype(np.float32)
    assert np.abs(const32 - exact).max() < 1e-4  # (what a float32 sum of terms of this size can lose)

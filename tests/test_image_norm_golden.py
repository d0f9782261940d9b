"""CPU: the image norms of the GMM patch prior (asinh, fixed-max, sigmoid, atan, log, power) against
tests/golden/image_norm.npz, generated from the LIVE reference by tools/make_golden_image_norm.py with the reference's
norm parameters held constant: host classes, oracle + norm, (de)serialisation, construction and the C ABI."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import rel_linf
from image_norm_cases import NEAR_TIE, NORM_CASES, SHAPE_CASES, cached_oracle, fixture_gmm, make_norm, oracle

from jolideco_amd import GMMPatchPrior, SpatialFluxComponent
from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
from jolideco_amd.utils import norms
from jolideco_amd.utils.io._fitsfile import read_fits

TYPES = list(NORM_CASES)


def test_fixture_covers_the_six_norms(golden):
    g = golden("image_norm")
    assert list(g["types"]) == TYPES and g["flux"].shape == (40, 44) and int(g["stride"]) == 4
    assert sorted(norms.NORMS_REGISTRY) == sorted(TYPES + ["identity"])
    for name in ("ASinhImageNorm", "FixedMaxImageNorm", "SigmoidImageNorm", "ATanImageNorm", "LogImageNorm", "PowerImageNorm"):
        assert name in norms.__all__ and issubclass(getattr(norms, name), norms.ImageNorm)


@pytest.mark.parametrize("type_", TYPES)
def test_host_norm_reproduces_the_reference_image(golden, type_):
    """Same torch ops as the reference on the same float32 parameters: exact on the generating torch build; 1 ulp is
    allowed for another build's vectorised asinh / atan / exp / log / pow."""
    g = golden("image_norm")
    norm = make_norm(type_)
    normed = norm(torch.from_numpy(g["flux"])).numpy()
    ref = g[f"{type_}/normed"]
    assert normed.dtype == np.float32
    assert np.all(np.abs(normed - ref) <= np.spacing(np.abs(ref)))
    assert np.array_equal(norm.evaluate_numpy(g["flux"].astype(np.float64)), normed)
    if type_ != "atan":  # (the reference's atan inverse leaves alpha out: not an inverse)
        flux = g["flux"] if type_ != "fixed-max" else np.minimum(g["flux"], 24.0)
        back = norm.inverse(norm(torch.from_numpy(flux))).numpy()
        np.testing.assert_allclose(back, flux, rtol=2e-5 if type_ != "sigmoid" else 2e-4)
        np.testing.assert_allclose(norm.inverse_numpy(norm.evaluate_numpy(flux)), flux, rtol=2e-5 if type_ != "sigmoid" else 2e-4)


@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("type_", TYPES)
def test_oracle_with_norm_reproduces_the_reference_prior(golden, type_, marginalize):
    """oracle/cpu_ref on norm(flux) = the reference's GMMPatchPrior(norm=..., cycle_spin=False): value and autograd
    gradient at the tolerances of tests/test_oracle_golden.py (bit for bit when the fixture was generated)."""
    g = golden("image_norm")
    total, dflux, _, _ = oracle(g["flux"], make_norm(type_), fixture_gmm(golden), 4, None, marginalize)
    scale = 16 / 64 / g["flux"].size
    tag = f"{type_}/{'lse' if marginalize else 'max'}"
    np.testing.assert_allclose(total * scale, float(g[f"{tag}/value"]), rtol=2e-6)
    assert rel_linf(dflux * scale, g[f"{tag}/grad"]) < (5e-4 if marginalize else 1e-5)
    assert np.abs(g[f"{tag}/grad"]).max() > 0


@pytest.mark.parametrize("type_", TYPES)
def test_near_ties_of_the_gpu_cases_stay_within_one_percent(golden, type_):
    """tests/test_gpu_image_norm.py may leave patches whose two best float64 log-likelihoods differ by less than 1e-3 out
    of the max-mode gradient comparison: at most 1 % of the patches of every case, on the oracle alone."""
    for index in range(len(SHAPE_CASES)):
        _, _, arg, margin = cached_oracle(golden, type_, index, False, np.float64)
        near = int((margin < NEAR_TIE).sum())
        assert near <= 0.01 * margin.size, (type_, SHAPE_CASES[index], near, margin.size)
        assert arg.size == margin.size > 0


@pytest.mark.parametrize("type_", TYPES)
def test_norm_dict_round_trip(type_):
    norm = make_norm(type_, frozen=True)
    data = norm.to_dict()
    assert data == dict({"type": type_}, **{k: float(np.float32(v)) for k, v in NORM_CASES[type_].items()})
    new = norms.ImageNorm.from_dict(data)
    assert type(new) is type(norm) and new.to_dict() == data and new.device_params() == norm.device_params()
    assert norm.frozen is True and new.frozen is False
    assert norm.device_params()[0] == TYPES.index(type_) + 1 == norm.device_kind


def test_reference_style_dict_builds_and_unsupported_norms_raise():
    norm = norms.ImageNorm.from_dict({"type": "asinh", "alpha": 3.0, "beta": 40.0})
    assert isinstance(norm, norms.ASinhImageNorm) and norm.device_params() == (1, 3.0, 40.0)
    assert norms.ASinhImageNorm().to_dict() == {"type": "asinh", "alpha": 1.0, "beta": 1.0}
    assert norms.IdentityImageNorm().device_params() == (0, 0.0, 0.0)
    for type_ in ("max", "inverse-cdf"):
        with pytest.raises(NotImplementedError):
            norms.ImageNorm.from_dict({"type": type_})


@pytest.fixture()
def gmm_library(tmp_path, monkeypatch, golden):
    """A user's GMM library directory with the fixture's mixture registered as "zoran-weiss"."""
    gmm = GaussianMixtureModel.from_numpy(*fixture_gmm(golden), meta=GaussianMixtureModelMeta(stride=4))
    gmm.write(tmp_path / "zw.fits")
    index = {"zoran-weiss": {"filename": "$JOLIDECO_GMM_LIBRARY/zw.fits", "format": "table"}}
    (tmp_path / "jolideco-gmm-library-index.json").write_text(json.dumps(index))
    monkeypatch.setenv("JOLIDECO_GMM_LIBRARY", str(tmp_path))
    return gmm


def test_prior_with_a_norm_constructs(golden):
    """Fails on the commit before the norms: `GMMPatchPrior` refused every norm but the identity."""
    gmm = GaussianMixtureModel.from_numpy(*fixture_gmm(golden), meta=GaussianMixtureModelMeta(stride=4))
    prior = GMMPatchPrior(gmm=gmm, norm=norms.ASinhImageNorm())
    assert prior.norm.to_dict() == {"type": "asinh", "alpha": 1.0, "beta": 1.0}
    assert prior.to_dict()["norm"] == prior.norm.to_dict()
    assert isinstance(GMMPatchPrior(gmm=gmm).norm, norms.IdentityImageNorm)

    class TableNorm(norms.ImageNorm):  # a norm without a device kernel is refused, never run some other way
        pass

    with pytest.raises(NotImplementedError):
        GMMPatchPrior(gmm=gmm, norm=TableNorm())


@pytest.mark.parametrize("format", ["fits", "yaml"])
@pytest.mark.parametrize("type_", TYPES)
def test_component_with_a_normed_prior_round_trips(type_, format, tmp_path, gmm_library):
    """Prior dict, YAML and FITS header carry the norm's type and parameters in the reference's layout
    (PNORMTYP / PNORMMAX / PNORMALP / PNORMBET, jolideco/utils/io/fits.py:16-37)."""
    prior = GMMPatchPrior(norm=make_norm(type_), marginalize=type_ == "log")
    assert GMMPatchPrior.from_dict(prior.to_dict()).norm.to_dict() == prior.norm.to_dict()
    component = SpatialFluxComponent(flux_upsampled=torch.ones((1, 1, 16, 16)), prior=prior)
    filename = tmp_path / f"component.{format}"
    component.write(filename=filename, format=format)
    new = SpatialFluxComponent.read(filename=filename, format=format)
    assert type(new.prior.norm) is type(prior.norm) and new.prior.norm.to_dict() == prior.norm.to_dict()
    assert new.prior.marginalize == prior.marginalize
    expected = prior.norm.to_dict()
    if format == "fits":
        header = read_fits(filename)[0].header
        assert header["PNORMTYP"] == type_
        for key, fits_key in (("max_value", "PNORMMAX"), ("alpha", "PNORMALP"), ("beta", "PNORMBET")):
            assert header.get(fits_key, None) == expected.get(key, None)
    else:
        text = filename.read_text()
        assert f"type: {type_}" in text and "!!python" not in text


def test_c_abi_of_the_image_norm():
    """The new symbol is exported and bound; a null handle or an unknown kind returns JD_ERR_INVALID with a message."""
    from jolideco_amd import _hip

    lib = _hip.lib()
    assert "jd_gmm_set_image_norm" in _hip.EXPORTS and hasattr(lib, "jd_gmm_set_image_norm")
    assert [name for name, _ in _hip.ImageNormStruct._fields_] == ["kind", "p0", "p1"]
    good = _hip.ImageNormStruct(1, 3.0, 40.0)
    assert lib.jd_gmm_set_image_norm(None, ctypes.byref(good)) == -1
    assert b"null argument" in lib.jd_last_error()
    assert lib.jd_gmm_set_image_norm(None, None) == -1
    assert b"null argument" in lib.jd_last_error()
    for kind in (7, -1):
        bad = _hip.ImageNormStruct(kind, 1.0, 1.0)
        assert lib.jd_gmm_set_image_norm(None, ctypes.byref(bad)) == -1
        assert b"unknown image norm kind" in lib.jd_last_error()


def test_c_abi_refuses_parameters_the_kernels_would_divide_by():
    """A zero scale (alpha, max_value; beta of the power and asinh norms) or a non-finite parameter is refused when the
    norm is set, with a message of its own -- not later, as NaNs in the images or a phase mismatch."""
    from jolideco_amd import _hip

    lib = _hip.lib()
    for kind, p0, p1 in [(1, 0.0, 1.0), (1, 3.0, 0.0), (2, 0.0, 0.0), (3, 0.0, 1.0), (4, 0.0, 0.0), (5, 0.0, 0.0), (6, 0.5, 0.0)]:
        bad = _hip.ImageNormStruct(kind, p0, p1)
        assert lib.jd_gmm_set_image_norm(None, ctypes.byref(bad)) == -1, (kind, p0, p1)
        assert b"divides" in lib.jd_last_error(), (kind, lib.jd_last_error())
    for kind, p0, p1 in [(1, float("nan"), 1.0), (3, 1.0, float("inf")), (6, float("-inf"), 2.0)]:
        bad = _hip.ImageNormStruct(kind, p0, p1)
        assert lib.jd_gmm_set_image_norm(None, ctypes.byref(bad)) == -1
        assert b"non-finite parameter" in lib.jd_last_error()
    # identity ignores its parameters; valid norms get as far as the handle check
    for kind, p0, p1 in [(0, float("nan"), 0.0), (6, 0.0, 2.0), (2, 24.0, 0.0), (5, -2.5, 0.0)]:
        ok = _hip.ImageNormStruct(kind, p0, p1)
        assert lib.jd_gmm_set_image_norm(None, ctypes.byref(ok)) == -1 and b"null argument" in lib.jd_last_error()

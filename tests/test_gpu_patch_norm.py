"""GPU: the GMM patch prior under the standardized patch norm, x = (p - mean(p)) / mean(p) ("std-subtract-mean"), fused
into the dense fp32 kernels (csrc/gmm_dense.hip for 8x8 patches, csrc/gmm256.hip for 16x16).

Oracle: tests/patch_norm_cases.py (the body of `cpu_ref.gmm_patch_log_like` with the other norm), pinned against the live
reference by tests/golden/patch_norm.npz.  Its float64 evaluation is the arbiter; the float32 oracle's own distance from
it, e_ref, sets the tolerances:
  D = 64   the protocol of tests/test_gpu_image_norm.py: value <= max(3e-6, 4 e_ref), gradient <= max(1e-5, 4 e_ref),
           arg-max equal on every patch whose float64 margin is at least NEAR_TIE = 1e-3, at most 1 % of patches left out;
  D = 256  the protocol of tests/test_gpu_gmm16.py: factor 4, floor 1e-6, arg-max equal where the float64 margin exceeds
           twice the measured absolute error of the kernel's log-probabilities.

Measured on an MI355X (profiles/patch_norm/README.md has every row).  D = 64: value at most 8.2e-8, gradient at most
3.1e-6 (logsumexp; its e_ref 2.3e-6).  D = 256: value 5.8e-8 to 6.4e-7 against an e_ref of 6.4e-8 to 9.6e-7 (the one-patch
case at shifts (4, -4), whose total is close to zero: 1.3e-5 against 4.3e-5); gradient at most 5.7e-7 against 4.2e-7
(logsumexp with dense factors 1.5e-6 against 7.6e-7).  Every case is inside its bound.

The D = 256 values are that close because the standardized passes add the residual of the constants
(jd_gmm_set_const_residual): a standardized patch's value (about 10 here) is c_k (about 90) minus q / 2 (about 80), and
the float32 c_k alone -- one number per component, its rounding of up to 2e-5 shared by every patch that picks it -- left
1e-6 to 4e-6 in the value, outside max(4 e_ref, 1e-6) for six of these cases.
"""
import numpy as np
import pytest
import torch

import patch_norm_cases as cases
from conftest import patch_cover_mask, rel_linf, unpack_datasets
from image_norm_cases import SHAPE_CASES, case_flux, fixture_gmm, rel_err
from tools import gmm16_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 4.0, 1e-6  # D = 256


def _std():
    from jolideco_amd.utils.norms import StandardizedSubtractMeanPatchNorm

    return StandardizedSubtractMeanPatchNorm()


def _model(arrays, stride=4, factors=None):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    if factors is not None:
        return GaussianMixtureModel(arrays[0], arrays[1], arrays[2], factors, meta=GaussianMixtureModelMeta(stride=stride))
    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


@pytest.fixture(scope="module")
def model(golden):
    return _model(fixture_gmm(golden))


@pytest.fixture(scope="module")
def model256():
    return _model(gmm16_cases.synthetic_mixture(gmm16_cases.K, gmm16_cases.SEED), stride=gmm16_cases.STRIDE)


def _n_patches(shape, stride, patch=8):
    return ((shape[0] - patch) // stride + 1) * ((shape[1] - patch) // stride + 1)


def _device_shifts(shifts, shape):
    from jolideco_amd.ops import DeviceShifts

    dev = torch.tensor([shifts[0] % shape[0], shifts[1] % shape[1]], dtype=torch.int32, device=DEV)
    return DeviceShifts(dev, shifts)


def _evaluate(model, flux, stride, shifts, marginalize=False, grad_init=None, coef=1.0, want_argmax=False, norm=None,
              patch_norm="std", **kwargs):
    """(value, gradient image, arg-max) of one low-level call with value scale 1 (the sum over the patches)"""
    if not torch.is_tensor(flux):
        flux = torch.from_numpy(np.ascontiguousarray(flux, dtype=np.float32)).to(DEV)
    handle = model.handle(DEV)
    value = torch.full((1,), np.nan, device=DEV)
    grad = torch.zeros_like(flux) if grad_init is None else grad_init.clone()
    patch = 8 if handle.D == 64 else 16
    argmax = torch.full((_n_patches(flux.shape, stride, patch),), -7, dtype=torch.int32, device=DEV) if want_argmax else None
    handle.prior_fwd_bwd(flux, stride, shifts, value, 1.0, grad=grad, grad_coef=coef, marginalize=marginalize,
                         argmax_out=argmax, norm=norm, patch_norm=_std() if patch_norm == "std" else patch_norm, **kwargs)
    torch.cuda.synchronize()
    return float(value), grad.cpu().numpy(), None if argmax is None else argmax.cpu().numpy()


def _check64(label, o64, o32, got, shape, stride, shifts, marginalize, g0=None, coef=1.0):
    """The D = 64 protocol (module docstring); `got` = (value, gradient accumulated into g0 with `coef`, arg-max)"""
    value, grad, argmax = got
    keep = np.ones(shape, dtype=bool)
    clear = None
    if not marginalize:
        clear = o64["margin"] >= cases.NEAR_TIE
        assert (~clear).sum() <= 0.01 * clear.size
        keep = ~patch_cover_mask(np.flatnonzero(~clear), shape, stride, shifts)
    e_ref_value = abs(o32["total"] - o64["total"]) / abs(o64["total"])
    e_ref_grad = rel_err(o32["grad"], o64["grad"], keep)
    e_value = abs(value - o64["total"]) / abs(o64["total"])
    expected = (0.0 if g0 is None else g0.astype(np.float64)) + coef * o64["grad"]
    e_grad = float(np.abs(grad - expected)[keep].max() / np.abs(coef * o64["grad"]).max())
    print(f"patch norm parity {label} {'lse' if marginalize else 'max'} {shape} stride {stride}: value e_ref {e_ref_value:.2e} "
          f"device {e_value:.2e} | gradient e_ref {e_ref_grad:.2e} device {e_grad:.2e}")
    assert np.abs(o64["grad"]).max() > 0 and np.isfinite(grad).all() and np.isfinite(value)
    assert e_value <= max(3e-6, 4 * e_ref_value)
    assert e_grad <= max(1e-5, 4 * e_ref_grad)
    if not marginalize:
        assert np.array_equal(argmax[clear], o64["arg"][clear])
        assert np.array_equal(argmax < 0, ~o64["keep"]), "the filtered patches differ"


def _log_prob_error(model, flux_np, stride, shifts, o64, patch):
    """max |kernel - float64| over the log-probabilities of the kept patches (estimate_log_prob on the standardized
    patches of the rolled image: the caller normalises explicit patches)"""
    rolled = np.roll(flux_np, tuple(int(s) for s in shifts), axis=(0, 1))
    x = cases.standardized_patches(rolled, patch, stride)[o64["keep"]]
    got = model.estimate_log_prob(torch.from_numpy(x).to(DEV)).cpu().numpy().astype(np.float64)
    return float(np.max(np.abs(got - o64["loglike"])))


def _check256(label, model, o64, o32, got, flux_np, stride, shifts, marginalize):
    """The D = 256 protocol (module docstring)"""
    value, grad, arg = got
    ref_v = abs(o32["total"] - o64["total"]) / abs(o64["total"])
    ref_g = rel_linf(o32["grad"], o64["grad"])
    err_v = abs(value - o64["total"]) / abs(o64["total"])
    err_g = rel_linf(grad, o64["grad"])
    print(f"patch norm gmm16 {label} shifts={shifts} {'lse' if marginalize else 'max'}: value kernel {err_v:.2e} fp32-oracle "
          f"{ref_v:.2e} | gradient kernel {err_g:.2e} fp32-oracle {ref_g:.2e}")
    if not marginalize:
        err_l = _log_prob_error(model, flux_np, stride, shifts, o64, 16)
        clear = o64["margin"] > 2.0 * err_l
        print(f"patch norm gmm16 {label}: log-prob abs error {err_l:.2e}, min margin {o64['margin'].min():.3g}, "
              f"{int((~clear).sum())} of {clear.size} patches under the margin")
        assert (~clear).mean() <= 0.01, "the inputs leave too many patches without a clear winner"
        assert np.array_equal(arg[clear], o64["arg"][clear]), "a wrong winner where the float64 margin is clear"
        assert np.array_equal(arg < 0, ~o64["keep"]), "the filtered patches differ"
    assert np.isfinite(value) and np.isfinite(grad).all()
    assert err_v <= max(FACTOR * ref_v, FLOOR), f"value: {err_v:.2e} > max(4 x {ref_v:.2e}, 1e-6)"
    assert err_g <= max(FACTOR * ref_g, FLOOR), f"gradient: {err_g:.2e} > max(4 x {ref_g:.2e}, 1e-6)"


# ------------------------------------------------------------------------------------------------ 1. parity, D = 64
@pytest.mark.parametrize("index", range(len(SHAPE_CASES)))
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("normed", [False, True])
def test_standardized_prior_matches_the_oracle(golden, model, normed, marginalize, index):
    """Value, arg-max and the gradient accumulated into a non-zero image with coef 0.75 against the float64 oracle."""
    shape, stride, shifts = SHAPE_CASES[index]
    o64 = cases.cached_oracle64(golden, index, marginalize, normed, np.float64)
    o32 = cases.cached_oracle64(golden, index, marginalize, normed, np.float32)
    g0 = np.random.RandomState(index).normal(size=shape).astype(np.float32) * np.float32(np.abs(o64["grad"]).max())
    coef = 0.75
    got = _evaluate(model, case_flux(index), stride, shifts, marginalize, torch.from_numpy(g0).to(DEV), coef,
                    want_argmax=not marginalize, norm=cases.asinh_norm() if normed else None)
    _check64("asinh" if normed else "identity", o64, o32, got, shape, stride, shifts, marginalize, g0, coef)


def test_fixture_values_of_the_reference(golden, model, model256):
    """The reference's own float32 numbers (tests/golden/patch_norm.npz), D = 64 and D = 256, at 1e-5."""
    g = golden("patch_norm")
    for d, mdl, flux, stride in ((64, model, case_flux(0), 4), (256, model256, gmm16_cases.fixture_flux(filtered=False), 8)):
        scale = stride**2 / d / flux.size
        for normed in (False, True):
            for marginalize in (False, True):
                value, grad, _ = _evaluate(mdl, flux, stride, None, marginalize, norm=cases.asinh_norm() if normed else None)
                tag = f"d{d}/{'asinh' if normed else 'bare'}/{'lse' if marginalize else 'max'}"
                assert value * scale == pytest.approx(float(g[f"{tag}/value"]), rel=1e-5), tag
                assert rel_linf(grad * scale, g[f"{tag}/grad"]) < 1e-5, tag


# ------------------------------------------------------------------------------------------------ 2. parity, D = 256
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("index", range(len(cases.SHAPES_256)))
def test_standardized_prior_on_16x16_patches_matches_the_oracle(model256, index, marginalize):
    shape, stride = cases.SHAPES_256[index]
    flux = cases.case_flux256(index)
    for shifts in cases.SHIFTS_256:
        o64 = cases.cached_oracle256(index, shifts, marginalize, "float64")
        o32 = cases.cached_oracle256(index, shifts, marginalize, "float32")
        got = _evaluate(model256, flux, stride, shifts, marginalize, want_argmax=not marginalize)
        _check256(f"{shape} stride {stride}", model256, o64, o32, got, flux, stride, shifts, marginalize)


# ------------------------------------------------------------------------------------------------ 3. non-triangular factors
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("d", [64, 256])
def test_factors_that_are_not_triangular(golden, d, marginalize):
    """Factors with a filled lower triangle (`gmm16_cases.dense_factors`) take the instantiations that skip nothing."""
    from jolideco_amd import _hip

    if d == 64:
        arrays, stride, shifts, shape = fixture_gmm(golden), 4, (2, -1), (37, 41)
        flux = np.random.RandomState(641).gamma(20, size=shape).astype(np.float32)
    else:
        arrays, stride, shifts, shape = gmm16_cases.synthetic_mixture(3, 1695), 8, (-3, 2), (45, 61)
        flux = gmm16_cases.case_flux(shape, 1697)
    factors = gmm16_cases.dense_factors(arrays, 1696)
    assert np.abs(np.tril(factors, -1)).max() > 0
    mdl = _model(arrays, stride=stride, factors=factors)
    assert _hip.lib().jd_gmm_is_triangular(mdl.handle(DEV)._handle) == 0
    o64 = cases.oracle(flux, arrays, stride, shifts, marginalize, np.float64, meta_stride=stride, factors=factors)
    o32 = cases.oracle(flux, arrays, stride, shifts, marginalize, np.float32, meta_stride=stride, factors=factors)
    got = _evaluate(mdl, flux, stride, shifts, marginalize, want_argmax=not marginalize)
    if d == 64:
        _check64("dense factors", o64, o32, got, shape, stride, shifts, marginalize)
    else:
        _check256("dense factors", mdl, o64, o32, got, flux, stride, shifts, marginalize)


# ------------------------------------------------------------------------------------------------ 4. filter
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("d", [64, 256])
def test_filtered_patch_contributes_nothing(golden, model, model256, d, marginalize):
    """One pixel at -2e5, covered by patch (0, 0) alone: the `> -1e5` filter acts on the patch before the norm.  The value
    is finite and the oracle's, and the pixels only that patch covers get a gradient of exactly 0."""
    if d == 64:
        mdl, arrays, stride, flux = model, fixture_gmm(golden), 4, case_flux(0).copy()
        flux[gmm16_cases.FILTERED_PIXEL] = -2e5
    else:
        mdl, arrays, stride = model256, gmm16_cases.synthetic_mixture(gmm16_cases.K, gmm16_cases.SEED), gmm16_cases.STRIDE
        flux = gmm16_cases.fixture_flux(filtered=True)
    o64 = cases.oracle(flux, arrays, stride, None, marginalize, np.float64, meta_stride=stride)
    o32 = cases.oracle(flux, arrays, stride, None, marginalize, np.float32, meta_stride=stride)
    assert int((~o64["keep"]).sum()) == 1 and not o64["keep"][0]
    got = _evaluate(mdl, flux, stride, (0, 0), marginalize, want_argmax=not marginalize)
    value, grad, arg = got
    assert np.isfinite(value) and abs(value) < 1e7  # (the filtered patch alone would add a term of the order of 1e10 or more)
    assert np.all(grad[:stride, :stride] == 0), "the filtered patch left a gradient on pixels only it covers"
    assert np.isfinite(grad).all() and np.any(grad[stride:, stride:] != 0)
    if not marginalize:
        assert arg[0] == -1 and np.all(arg[1:] >= 0)
    if d == 64:
        _check64("filter", o64, o32, got, flux.shape, stride, (0, 0), marginalize)
    else:
        _check256("filter", mdl, o64, o32, got, flux, stride, (0, 0), marginalize)


# ------------------------------------------------------------------------------------------------ 5. path equivalences
EQUIV_SHAPES = [(72, 100), (37, 41)]


def _equiv_flux(shape):
    return torch.from_numpy(np.random.RandomState(shape[0]).gamma(20, size=shape).astype(np.float32)).to(DEV)


def _same(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.abs(a[1]).max() > 0
    if a[2] is not None:
        assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("shape", EQUIV_SHAPES)
def test_kernel_paths_agree_bit_for_bit(golden, jd_option, shape, marginalize):
    """Everything behind the gradient rows is shared with the subtract-mean prior and works unchanged: phase 1 then
    phase 2 = one call, device-resident shifts = by-value shifts, per-pixel = tiled gather; and the screen switches
    change nothing, because the standardized norm never takes the screen (its generation does not advance)."""
    mdl = _model(fixture_gmm(golden))  # a handle of its own: no screened pass has ever run on it
    handle = mdl.handle(DEV)
    flux, shifts = _equiv_flux(shape), (3, -2)
    g0 = torch.from_numpy(np.random.RandomState(1).normal(size=shape).astype(np.float32)).to(DEV)

    def run(**kwargs):
        return _evaluate(mdl, flux, 4, kwargs.pop("shifts", shifts), marginalize, g0, -0.7, want_argmax=not marginalize, **kwargs)

    base = run()
    _same(run(shifts=_device_shifts(shifts, shape)), base)
    jd_option("JD_GMM_GATHER_TILED", 0)
    _same(run(), base)
    jd_option("JD_GMM_GATHER_TILED", None)
    for key in ("JD_GMM_SCREEN", "JD_GMM_LSE_SCREEN"):
        for setting in (0, 2, None):
            jd_option(key, setting)
            _same(run(), base)
    assert handle.screen_stats()[0] == 0, "a screened pass ran under the standardized patch norm"
    # phase 1 (value, rows: reads the flux only), then phase 2 (gather) with the same arguments
    value, grad = torch.zeros(1, device=DEV), g0.clone()
    for phases in (1, 2):
        handle.prior_fwd_bwd(flux, 4, shifts, value, 1.0, grad=grad, grad_coef=-0.7, marginalize=marginalize, patch_norm=_std(),
                             phases=phases)
        if phases == 1:
            torch.cuda.synchronize()
            assert np.array_equal(grad.cpu().numpy(), g0.cpu().numpy())  # phase 1 does not touch the gradient image
    torch.cuda.synchronize()
    _same((float(value), grad.cpu().numpy(), None), base)
    # a phase 2 after a phase 1 under the other patch norm is refused, both ways
    for first, second in ((_std(), None), (None, _std())):
        handle.prior_fwd_bwd(flux, 4, shifts, value, 1.0, grad=grad, grad_coef=-0.7, marginalize=marginalize, patch_norm=first, phases=1)
        with pytest.raises(RuntimeError, match="matching phase 1"):
            handle.prior_fwd_bwd(flux, 4, shifts, value, 1.0, grad=grad, grad_coef=-0.7, marginalize=marginalize, patch_norm=second,
                                 phases=2)
    # ... and the subtract-mean prior on the same handle is another function (and does take the screen)
    other = run(patch_norm=None)
    assert other[0] != base[0] and not np.array_equal(other[1], base[1])


@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("shape", EQUIV_SHAPES)
def test_band_of_a_row_shard_equals_the_accumulating_call(model, shape, marginalize):
    """The band of patch rows (3, n - 2) added into a zero image by jd_add_rolled_bands is the accumulating call of the
    same rows, bit for bit."""
    from jolideco_amd.ops import add_rolled_bands, band_rows

    flux, shifts = _equiv_flux(shape), (-2, 3)
    handle = model.handle(DEV)
    rows = (3, (shape[0] - 8) // 4 + 1 - 2)
    y0, y1 = band_rows(rows, 4, shape[0])
    ref_v, ref_g = torch.zeros(1, device=DEV), torch.zeros_like(flux)
    handle.prior_fwd_bwd(flux, 4, shifts, ref_v, 0.25, grad=ref_g, grad_coef=-0.7, patch_rows=rows, marginalize=marginalize,
                         patch_norm=_std())
    band = torch.full(((y1 - y0) * shape[1] + 4,), 7.0, device=DEV)
    v = torch.zeros(1, device=DEV)
    handle.prior_fwd_bwd(flux, 4, shifts, v, 0.25, grad_coef=-0.7, patch_rows=rows, marginalize=marginalize, band_out=band,
                         patch_norm=_std())
    grad = torch.zeros_like(flux)
    add_rolled_bands(grad, shifts, band, band.numel(), [(y0, y1)])
    torch.cuda.synchronize()
    assert np.array_equal(grad.cpu().numpy(), ref_g.cpu().numpy()) and np.abs(ref_g.cpu().numpy()).max() > 0
    assert float(v) == float(ref_v)
    whole = _evaluate(model, flux, 4, shifts, marginalize, coef=-0.7)
    assert not np.array_equal(whole[1], ref_g.cpu().numpy())  # (the shard is a proper part)


# ------------------------------------------------------------------------------------------------ 6. optimizer step
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_optimizer_step_in_the_gather_changes_no_bit(model, monkeypatch, optimizer):
    """`device_fwd_bwd_step` (the gather applies the optimizer step) against `device_fwd_bwd` followed by the stand-alone
    step (JOLIDECO_NO_FUSED_STEP=1): 3 joint epochs, fluxes and every trace column bit for bit."""
    from jolideco_amd import GMMPatchPrior, MAPDeconvolver, SpatialFluxComponent
    from jolideco_amd.data import synthetic_observations

    datasets, _, flux_init = synthetic_observations(shape=(72, 100), n_obs=2, seed=4)
    results = {}
    for mode in ("fused", "separate"):
        if mode == "separate":
            monkeypatch.setenv("JOLIDECO_NO_FUSED_STEP", "1")
        comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=GMMPatchPrior(gmm=model, patch_norm=_std()))
        kwargs = {"optimizer_type": optimizer}
        if optimizer == "sgd":
            kwargs["learning_rate"] = 1e-3
        deco = MAPDeconvolver(n_epochs=3, display_progress=False, device=DEV, fit_mode="joint", **kwargs)
        session = deco.session(datasets, components=comp)
        assert session._fuse_step(session.states[0], session.priors[0]) == (mode == "fused")
        res = deco.run(datasets, components=comp)
        results[mode] = (res.flux_total, {n: np.asarray(res.trace_loss[n]) for n in res.trace_loss.colnames if n != "filename"})
    assert np.array_equal(results["fused"][0], results["separate"][0])
    assert not np.array_equal(results["fused"][0], flux_init.astype(np.float32)) and np.isfinite(results["fused"][0]).all()
    for name, column in results["separate"][1].items():
        assert np.array_equal(results["fused"][1][name], column), name


# ------------------------------------------------------------------------------------------------ 7. shared handle
def test_two_priors_with_different_patch_norms_share_one_handle(golden, model):
    """`gmm.handle(device)` is cached per mixture: the patch norm travels with every call, so a standardized and a
    subtract-mean prior evaluated alternately each give their own single-prior result, bit for bit."""
    from jolideco_amd import GMMPatchPrior
    from jolideco_amd.utils.norms import SubtractMeanPatchNorm

    flux = _equiv_flux((72, 100))
    norms_ = {"std": _std(), "mean": SubtractMeanPatchNorm()}
    priors = {name: GMMPatchPrior(gmm=model, patch_norm=n, cycle_spin=False) for name, n in norms_.items()}
    assert priors["std"].gmm.handle(DEV) is priors["mean"].gmm.handle(DEV)

    def run(prior):
        value, grad = torch.zeros(1, device=DEV), torch.zeros_like(flux)
        prior.device_fwd_bwd(flux, value, grad=grad, coef=-1.0, shifts=(1, 2))
        torch.cuda.synchronize()
        return float(value), grad.cpu().numpy()

    # a handle of its own each
    single = {name: run(GMMPatchPrior(gmm=_model(fixture_gmm(golden)), patch_norm=n, cycle_spin=False)) for name, n in norms_.items()}
    assert single["std"][0] != single["mean"][0] and not np.array_equal(single["std"][1], single["mean"][1])
    for name in ("std", "mean", "std", "mean", "mean", "std"):
        value, grad = run(priors[name])
        assert value == single[name][0] and np.array_equal(grad, single[name][1]), name


def test_residual_of_the_constants_enters_the_standardized_pass_only(model256):
    """A handle without the residual (`GmmHandle` built by hand, as before the norm) and the mixture's own handle, which
    carries it: the subtract-mean pass has the same bits on both; the standardized value moves by the residual of the
    winning components, a few 1e-6 of it, and its gradient (max mode: no l enters it) keeps its bits."""
    from jolideco_amd.ops import GmmHandle

    class Bare:  # (what `_evaluate` needs of a mixture)
        def __init__(self, gmm):
            self._handle = GmmHandle(gmm.precisions_cholesky_numpy, gmm.means_precisions_cholesky_numpy, gmm.log_det_cholesky_numpy,
                                     gmm.log_weights_numpy, gmm.pixel_weights_numpy.astype(np.float32), torch.device(DEV))

        def handle(self, device):
            return self._handle

    bare, flux = Bare(model256), gmm16_cases.case_flux((40, 56), 1650)
    for marginalize in (False, True):
        a = _evaluate(bare, flux, 8, (1, 2), marginalize, patch_norm=None, want_argmax=not marginalize)
        b = _evaluate(model256, flux, 8, (1, 2), marginalize, patch_norm=None, want_argmax=not marginalize)
        _same(a, b)
    a = _evaluate(bare, flux, 8, (1, 2), want_argmax=True)
    b = _evaluate(model256, flux, 8, (1, 2), want_argmax=True)
    assert a[0] != b[0] and abs(a[0] - b[0]) < 1e-5 * abs(b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    bare._handle.close()


# ------------------------------------------------------------------------------------------------ 8. autograd
@pytest.mark.parametrize("d", [64, 256])
def test_autograd_equals_the_fused_path(model, model256, d):
    """`prior(flux).backward()`: the library returns the finished flux gradient."""
    from jolideco_amd import GMMPatchPrior

    prior = GMMPatchPrior(gmm=model if d == 64 else model256, patch_norm=_std(), cycle_spin=False)
    flux = _equiv_flux((37, 41)).reshape(1, 1, 37, 41).requires_grad_(True)
    value = prior(flux)
    value.backward()
    ref_v, ref_g = torch.zeros(1, device=DEV), torch.zeros((37, 41), device=DEV)
    prior.device_fwd_bwd(flux.detach(), ref_v, grad=ref_g, coef=1.0, shifts=None)
    torch.cuda.synchronize()
    assert float(value.detach()) == pytest.approx(float(ref_v), rel=1e-6)
    assert rel_linf(flux.grad.cpu().numpy()[0, 0], ref_g.cpu().numpy()) < 1e-6 and np.abs(ref_g.cpu().numpy()).max() > 0


# ------------------------------------------------------------------------------------------------ 9. fits
def _fit_inputs(golden):
    from jolideco_amd import GMMPatchPrior, SpatialFluxComponent

    g = golden("patch_norm")
    arrays = tuple(np.asarray(g[f"fit/gmm/{name}"], dtype=np.float64) for name in ("means", "covariances", "weights"))
    comp = SpatialFluxComponent.from_numpy(flux=g["fit/flux_init"], prior=GMMPatchPrior(gmm=_model(arrays), patch_norm=_std()))
    return g, unpack_datasets(g, "fit/data/"), comp


def test_fit_matches_the_reference(golden):
    """6 sequential epochs, 32 x 32, cycle-spin on with the default generator: final flux and trace of the reference at
    the tolerances tests/test_gpu_fit.py holds its reference-generated fits to."""
    from jolideco_amd import MAPDeconvolver

    g, datasets, comp = _fit_inputs(golden)
    res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).run(datasets, components=comp)
    err = rel_linf(res.flux_total, g["fit/flux_final"])
    print("patch norm fit rel Linf", err)
    assert err < 1e-5
    for key, ref in g.items():
        if key.startswith("fit/trace/"):
            name = key[len("fit/trace/"):]
            np.testing.assert_allclose(res.trace_loss[name], ref, rtol=2e-5, atol=1e-6, err_msg=name)


def test_replayed_epochs_equal_the_by_value_epochs(golden, monkeypatch):
    """Captured epochs (JOLIDECO_GRAPH=1) = by-value epochs, bit for bit, with at least one graph captured."""
    from jolideco_amd import MAPDeconvolver

    out = {}
    for mode in ("host", "graph"):
        monkeypatch.setenv("JOLIDECO_STEP_SCALARS", "host" if mode == "host" else "device")
        monkeypatch.setenv("JOLIDECO_GRAPH", "1" if mode == "graph" else "0")
        _, datasets, comp = _fit_inputs(golden)
        session = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).session(datasets, components=comp)
        rows = []
        for _ in range(cases.FIT_EPOCHS):
            session.epoch()
            rows.append(session.scalars.clone())
        torch.cuda.synchronize()
        out[mode] = (session.states[0].flux_cur.cpu().numpy().copy(), torch.stack(rows).cpu().numpy(), len(session._graphs))
    assert out["host"][2] == 0 and out["graph"][2] >= 1, "no epoch was captured"
    assert np.array_equal(out["graph"][0], out["host"][0]) and np.array_equal(out["graph"][1], out["host"][1])


def test_fit_on_16x16_patches_runs(golden):
    """3 sequential epochs at 48 x 48 with a 16x16 mixture: finite, and the flux moves."""
    from jolideco_amd import GMMPatchPrior, MAPDeconvolver, SpatialFluxComponent

    g = golden("gmm16")
    arrays = gmm16_cases.synthetic_mixture(gmm16_cases.FIT_K, gmm16_cases.FIT_GMM_SEED)
    prior = GMMPatchPrior(gmm=_model(arrays, stride=gmm16_cases.STRIDE), patch_norm=_std())
    comp = SpatialFluxComponent.from_numpy(flux=g["fit/flux_init"], prior=prior)
    res = MAPDeconvolver(n_epochs=3, display_progress=False, device=DEV).run(unpack_datasets(g, "fit/data/"), components=comp)
    assert res.flux_total.shape == gmm16_cases.FIT_SHAPE and np.isfinite(res.flux_total).all()
    assert np.isfinite(np.asarray(res.trace_loss["total"])).all()
    assert rel_linf(res.flux_total, g["fit/flux_init"]) > 1e-3

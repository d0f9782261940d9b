"""GPU: sub-pixel cycle spin of InverseGammaPrior / ExponentialPrior (jd_elementwise_prior_subpix_fwd_bwd) and SmoothnessPrior
(jd_smoothness_prior_fwd_bwd) against the float64 oracles of tests/prior_cases.py (pinned against the live reference when
tools/make_golden_priors.py generated tests/golden/priors.npz), the fixture itself, and -- for fits -- the by-value epochs.

Bound of the kernel tests, the project's rule: the error against float64 is at most 4 x the float32 CPU oracle's own error
against float64, floor 1e-6 (relative L-infinity; for a value: relative difference).  Every case prints both figures."""
from ctypes import c_float

import numpy as np
import pytest
import torch

import prior_cases as cases
from conftest import rel_linf, unpack_datasets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(array):
    return torch.tensor(np.ascontiguousarray(array, dtype=np.float32), device=DEV)


def _subpix_raw(kind, flux, x0, y0, coef, grad=None, offset_dev=None):
    """One call of the C entry on device tensors; returns the value (the gradient is accumulated into `grad`)."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, stream_ptr

    params = cases.SPARSE_PARAMS[kind]
    alpha, beta = params["alpha"], params.get("beta", 0.0)
    H, W = flux.shape
    value = torch.empty(1, dtype=torch.float32, device=DEV)
    check(_hip.lib().jd_elementwise_prior_subpix_fwd_bwd(
        cases.KINDS[kind], ptr(flux), H, W, c_float(alpha), c_float(beta), c_float(cases.log_constant(kind, alpha, beta)),
        c_float(x0), c_float(y0), ptr(offset_dev), ptr(value), c_float(coef), ptr(grad), stream_ptr(flux.device)))
    return value


def _value_error(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("shape", cases.SUBPIX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_subpix_kernel_against_float64(kind, shape):
    flux_np = cases.case_flux(shape)
    flux = _dev(flux_np)
    n = flux_np.size
    for offsets in cases.SUBPIX_OFFSETS:
        value64, grad64 = cases.cached_sparse_oracle(shape, kind, offsets, "float64")
        value32, grad32 = cases.cached_sparse_oracle(shape, kind, offsets, "float32")
        own_v, own_g = _value_error(value32, value64), rel_linf(grad32, grad64)
        grad = torch.zeros_like(flux)
        value = _subpix_raw(kind, flux, *offsets, 1.0 / n, grad)
        # from device memory, with by-value arguments the kernel must not read
        grad_dev = torch.zeros_like(flux)
        value_dev = _subpix_raw(kind, flux, 0.0, 0.0, 1.0 / n, grad_dev, offset_dev=_dev(offsets))
        value_only = _subpix_raw(kind, flux, *offsets, 1.0 / n, None)
        torch.cuda.synchronize()
        err_v, err_g = _value_error(value.item(), value64), rel_linf(grad.cpu().numpy(), grad64)
        print(f"subpix {kind} {shape} {offsets}: value err {err_v:.2e} (float32 oracle {own_v:.2e}), "
              f"grad err {err_g:.2e} (float32 oracle {own_g:.2e})")
        assert err_v <= cases.bound(own_v), (offsets, err_v, own_v)
        assert err_g <= cases.bound(own_g), (offsets, err_g, own_g)
        assert torch.equal(grad, grad_dev) and torch.equal(value, value_dev), f"{offsets}: device offsets differ from by-value"
        assert torch.equal(value, value_only), f"{offsets}: value-only call differs"


@pytest.mark.parametrize("shape", [(33, 65), (64, 96), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_zero_offsets_equal_the_plain_kernel(kind, shape):
    """(0, 0): the stencil is 1 x f plus exact zeros -- the gradient has the bits of jd_elementwise_prior_fwd_bwd, the value
    (another partition of the same double sum) is within 1 ulp."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, stream_ptr

    flux = _dev(cases.case_flux(shape))
    n = flux.numel()
    params = cases.SPARSE_PARAMS[kind]
    alpha, beta = params["alpha"], params.get("beta", 0.0)
    noise = _dev(np.random.RandomState(5).normal(size=shape))
    grad_plain, value_plain = noise.clone(), torch.empty(1, dtype=torch.float32, device=DEV)
    check(_hip.lib().jd_elementwise_prior_fwd_bwd(
        cases.KINDS[kind], ptr(flux), n, c_float(alpha), c_float(beta), c_float(cases.log_constant(kind, alpha, beta)),
        ptr(value_plain), c_float(-0.7 / n), ptr(grad_plain), stream_ptr(flux.device)))
    grad = noise.clone()
    value = _subpix_raw(kind, flux, 0.0, 0.0, -0.7 / n, grad)
    torch.cuda.synchronize()
    assert torch.equal(grad, grad_plain)
    ulp = np.spacing(np.float32(abs(value_plain.item())))
    assert abs(value.item() - value_plain.item()) <= ulp, (value.item(), value_plain.item())


@pytest.mark.parametrize("shape", [(33, 65), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_gradient_is_accumulated_once_per_pixel(kind, shape):
    """grad pre-filled with noise receives old + coef * df; a second run from the same state gives the same bits."""
    offsets = (-0.25, 0.4)
    flux = _dev(cases.case_flux(shape))
    n = flux.numel()
    coef = -0.7
    _, grad64 = cases.cached_sparse_oracle(shape, kind, offsets, "float64")
    _, grad32 = cases.cached_sparse_oracle(shape, kind, offsets, "float32")
    scale = np.abs(grad64).max() * abs(coef)
    old = (np.random.RandomState(6).normal(size=shape) * scale).astype(np.float32)
    expected = old.astype(np.float64) + coef * grad64
    own = rel_linf(old + np.float32(coef) * grad32.astype(np.float32), expected)
    runs = []
    for _ in range(2):
        grad = _dev(old)
        _subpix_raw(kind, flux, *offsets, coef / n, grad)
        runs.append(grad)
    torch.cuda.synchronize()
    err = rel_linf(runs[0].cpu().numpy(), expected)
    print(f"subpix accumulate {kind} {shape}: err {err:.2e} (float32 oracle {own:.2e})")
    assert err <= cases.bound(own), (err, own)
    assert torch.equal(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_sparse_priors_match_the_fixture(golden, kind):
    import jolideco_amd as jd

    g = golden("priors")
    cls = jd.InverseGammaPrior if kind == "inverse-gamma" else jd.ExponentialPrior
    flux = _dev(g["flux"])[None, None]
    prior = cls(cycle_spin_subpix=True, generator=torch.Generator("cpu").manual_seed(cases.FIXTURE_SEED),
                **cases.SPARSE_PARAMS[kind])
    f = flux.clone().requires_grad_(True)
    value = prior(f)  # the autograd seam: draws the fixture's offsets
    value.backward()
    assert prior.last_shifts == tuple(g[f"{kind}/offsets"])
    assert _value_error(value.item(), g[f"{kind}/value"]) < 1e-5
    assert rel_linf(f.grad.cpu().numpy()[0, 0], g[f"{kind}/grad"]) < 1e-5
    # the fused path with the same offsets: same bits
    out, grad = torch.empty(1, dtype=torch.float32, device=DEV), torch.zeros_like(flux)
    prior.device_fwd_bwd(flux, out, grad=grad, coef=1.0, shifts=prior.last_shifts)
    assert out.item() == value.item() and torch.equal(grad, f.grad)


@pytest.mark.parametrize("width", cases.SMOOTH_WIDTHS)
def test_smoothness_prior_matches_the_fixture(golden, width):
    import jolideco_amd as jd

    g = golden("priors")
    flux = _dev(g["flux"])[None, None]
    prior = jd.SmoothnessPrior(width=width)
    f = flux.clone().requires_grad_(True)
    value = prior(f)
    value.backward()
    assert _value_error(value.item(), g[f"smooth/{width}/value"]) < 1e-5
    assert rel_linf(f.grad.cpu().numpy()[0, 0], g[f"smooth/{width}/grad"]) < 1e-5


@pytest.mark.parametrize("tag", ["fit_subpix", "fit_smooth"])
def test_fits_match_the_fixture(golden, tag):
    import jolideco_amd as jd

    g = golden("priors")
    datasets = unpack_datasets(g, prefix=f"{tag}/data/")
    prior = jd.InverseGammaPrior(cycle_spin_subpix=True) if tag == "fit_subpix" else jd.SmoothnessPrior()
    comp = jd.SpatialFluxComponent.from_numpy(flux=g[f"{tag}/flux_init"], prior=prior)
    res = jd.MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).run(datasets, components=comp)
    err = rel_linf(res.flux_total, g[f"{tag}/flux_final"])
    print(f"{tag}: flux rel Linf {err:.2e}")
    assert err < 1e-5
    np.testing.assert_allclose(res.trace_loss["total"], g[f"{tag}/trace/total"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------------- epoch forms
def _gmm(k=8, seed=2):
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    means, covs, weights = synthetic_gmm(k, 64, seed=seed)
    return GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))


def _build_points():
    from jolideco_amd import InverseGammaPrior, SpatialFluxComponent
    from jolideco_amd.data import synthetic_observations

    datasets, _, flux_init = synthetic_observations(shape=(40, 72), n_obs=3, seed=3)
    prior = InverseGammaPrior(cycle_spin_subpix=True, generator=torch.Generator().manual_seed(5))
    return datasets, SpatialFluxComponent.from_numpy(flux=0.05 * flux_init, prior=prior)


def _build_mixed():
    from jolideco_amd import FluxComponents, GMMPatchPrior, InverseGammaPrior, SpatialFluxComponent
    from jolideco_amd.data import gaussian_kernel, synthetic_observations

    datasets, _, flux_init = synthetic_observations(shape=(72, 88), n_obs=3, seed=4)
    comps = FluxComponents()
    comps["extended"] = SpatialFluxComponent.from_numpy(
        flux=flux_init, prior=GMMPatchPrior(gmm=_gmm(), generator=torch.Generator().manual_seed(11)))
    comps["points"] = SpatialFluxComponent.from_numpy(
        flux=0.05 * flux_init, prior=InverseGammaPrior(cycle_spin_subpix=True, generator=torch.Generator().manual_seed(12)))
    for i, d in enumerate(datasets.values()):
        d["psf"] = {"extended": d["psf"], "points": gaussian_kernel(1.0 + 0.1 * i, (9, 9)).astype(np.float32)}
    return datasets, comps


def _fit(monkeypatch, mode, build, n_epochs, fit_mode):
    """mode: "host" (by value), "device" (planned, no capture), "graph" (planned + captured)."""
    from jolideco_amd import MAPDeconvolver

    monkeypatch.setenv("JOLIDECO_STEP_SCALARS", "host" if mode == "host" else "device")
    monkeypatch.setenv("JOLIDECO_GRAPH", "1" if mode == "graph" else "0")
    datasets, components = build()
    session = MAPDeconvolver(n_epochs=n_epochs, display_progress=False, device=DEV, fit_mode=fit_mode).session(
        datasets, components=components)
    rows = []
    for _ in range(n_epochs):
        session.epoch()
        rows.append(session.scalars.clone())
    torch.cuda.synchronize()
    fluxes = [st.flux_cur.cpu().numpy().copy() for st in session.states]
    host = [(p.last_shifts, p.generator.get_state().numpy().tobytes()) for p in session.priors]
    return fluxes, torch.stack(rows).cpu().numpy(), host, len(session._graphs), session.step


@pytest.mark.parametrize("case", ["points-sequential", "points-joint", "mixed-joint"])
def test_planned_and_replayed_epochs_equal_the_by_value_epochs(monkeypatch, case):
    """By value, planned (offsets in the device slots of `StepScalars`) and replayed from a captured graph: the same flux bit
    for bit, the same trace scalars, the generators in the same state.  "mixed": a GMM 8 x 8 prior on one layer, the sub-pixel
    inverse-gamma prior on the other, in one joint fit."""
    name, fit_mode = case.split("-")
    build = _build_points if name == "points" else _build_mixed
    n_epochs = 9  # three eager epochs, a capture per flux-buffer parity, replays
    by_value = _fit(monkeypatch, "host", build, n_epochs, fit_mode)
    planned = _fit(monkeypatch, "device", build, n_epochs, fit_mode)
    replayed = _fit(monkeypatch, "graph", build, n_epochs, fit_mode)
    assert by_value[3] == 0 and planned[3] == 0 and replayed[3] >= 1, "no epoch was captured"
    assert np.all(np.isfinite(by_value[1])) and all(np.all(np.isfinite(f)) for f in by_value[0])
    for other in (planned, replayed):
        for a, b in zip(other[0], by_value[0]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(other[1], by_value[1])
        assert other[2] == by_value[2] and other[4] == by_value[4]


# ---------------------------------------------------------------------------------------------------- smoothness prior
@pytest.mark.parametrize("method", ["separable", "fft"])
@pytest.mark.parametrize("shape,width", cases.SMOOTH_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"w{v}")
def test_smoothness_prior_against_float64(monkeypatch, shape, width, method):
    import jolideco_amd as jd

    monkeypatch.setenv("JOLIDECO_CONV_METHOD", method)
    flux_np = cases.case_flux(shape, seed=7)
    value64, grad64 = cases.cached_smoothness_oracle(shape, width, "float64")
    value32, grad32 = cases.cached_smoothness_oracle(shape, width, "float32")
    own_v, own_g = _value_error(value32, value64), rel_linf(grad32, grad64)
    prior = jd.SmoothnessPrior(width=width)
    flux = _dev(flux_np)[None, None]
    plan, _ = prior._operator(flux)
    assert plan.method == method
    value, grad = torch.empty(1, dtype=torch.float32, device=DEV), torch.zeros_like(flux)
    prior.device_fwd_bwd(flux, value, grad=grad, coef=1.0)
    value_only = torch.empty(1, dtype=torch.float32, device=DEV)
    prior.device_fwd_bwd(flux, value_only)
    f = flux.clone().requires_grad_(True)
    seam = prior(f)
    seam.backward()
    torch.cuda.synchronize()
    err_v, err_g = _value_error(value.item(), value64), rel_linf(grad.cpu().numpy()[0, 0], grad64)
    print(f"smoothness {shape} width {width} {method}: value err {err_v:.2e} (float32 oracle {own_v:.2e}), "
          f"grad err {err_g:.2e} (float32 oracle {own_g:.2e})")
    assert err_v <= cases.bound(own_v), (err_v, own_v)
    assert err_g <= cases.bound(own_g), (err_g, own_g)
    # the autograd seam equals the fused path
    assert value_only.item() == value.item() == seam.item() and torch.equal(f.grad, grad)
    hess = prior.hessian_ones(flux)
    ones64 = cases.smoothness_oracle(np.ones(shape), cases.gaussian_kernel(width), np.float64)[1]  # -2 K (*) 1
    assert rel_linf(hess.cpu().numpy()[0, 0], ones64) < 1e-5

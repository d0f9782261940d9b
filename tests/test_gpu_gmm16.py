"""GPU: the GMM patch prior on 16x16 patches (256 features; jolideco_amd/csrc/gmm256.hip) against `oracle/cpu_ref` and
tests/golden/gmm16.npz (generated from the live reference by tools/make_golden_gmm16.py).

Tolerances are measured, not chosen: for every parity case the oracle runs in float64 and in float32 on the CPU, and
the kernel's relative L-infinity error against float64 may be at most FACTOR = 4 times the float32 oracle's own error
against float64 (another summation order over 256 terms and over K), with a floor of 1e-6 -- for the value and the
gradient separately.  The arg-max must equal the float64 arg-max on every patch whose float64 margin (best minus
runner-up) exceeds twice the measured absolute error of the kernel's log-probabilities; at most 1 % of the patches of a
case may lie under that margin.  The figures measured on an MI355X are in profiles/gmm16/README.md."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_linf, unpack_datasets
from tools import gmm16_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 4.0, 1e-6
SHIFTS = [(0, 0), (4, -4), (-3, 2)]
# (shape, stride): one patch | several tiles' worth of overlap | uncovered right and bottom pixels | no overlap |
# odd stride with ragged coverage
SHAPE_CASES = [((16, 16), 8), ((40, 56), 8), ((45, 61), 8), ((48, 48), 16), ((37, 50), 5)]


def _model(arrays, stride=cases.STRIDE):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(k, seed):
        if (k, seed) not in cache:
            cache[(k, seed)] = _model(cases.synthetic_mixture(k, seed))
        return cache[(k, seed)]

    return get


def _device_shifts(shifts, shape):
    from jolideco_amd.ops import DeviceShifts

    dev = torch.tensor([shifts[0] % shape[0], shifts[1] % shape[1]], dtype=torch.int32, device=DEV)
    return DeviceShifts(dev, shifts)


def _run(model, flux_np, stride, shifts, marginalize, norm=None, on_device=False, want_grad=True):
    """(sum of the per-patch values, gradient of that sum, arg-max per patch) from the library, scale 1"""
    flux = torch.from_numpy(np.ascontiguousarray(flux_np, dtype=np.float32)).to(DEV)
    value = torch.full((1,), np.nan, device=DEV)
    grad = torch.zeros_like(flux) if want_grad else None
    arg = None if marginalize else torch.full((cases.n_patches(flux_np.shape, stride),), -7, dtype=torch.int32, device=DEV)
    sh = _device_shifts(shifts, flux_np.shape) if on_device else shifts
    model.handle(DEV).prior_fwd_bwd(flux, stride, sh, value, 1.0, grad=grad, grad_coef=1.0, marginalize=marginalize,
                                    argmax_out=arg, norm=norm)
    torch.cuda.synchronize()
    return (float(value), None if grad is None else grad.cpu().numpy(), None if arg is None else arg.cpu().numpy())


def _log_prob_error(model, flux_np, stride, shifts, o64, norm=None):
    """max |kernel - float64| over the log-probabilities of the case's kept patches (estimate_log_prob on the mean-free
    patches of the rolled [normed] image)"""
    image = torch.from_numpy(flux_np.astype(np.float64))
    if norm is not None:
        image = norm(image)
    rolled = torch.roll(image, shifts=tuple(int(s) for s in shifts), dims=(0, 1)).numpy()
    x = cases.mean_free_patches(rolled.astype(np.float32), stride)[o64["keep"]]
    got = model.estimate_log_prob(torch.from_numpy(x).to(DEV)).cpu().numpy().astype(np.float64)
    # (the float32 rounding of the rolled image's patches is part of what the kernel sees; o64 saw the same float32 flux)
    return float(np.max(np.abs(got - o64["loglike"])))


def _check_case(model, arrays, flux_np, stride, shifts, marginalize, norm=None, label="", got=None):
    o64 = cases.oracle(flux_np, arrays, stride, shifts, marginalize, np.float64, norm=norm)
    o32 = cases.oracle(flux_np, arrays, stride, shifts, marginalize, np.float32, norm=norm)
    value, grad, arg = got if got is not None else _run(model, flux_np, stride, shifts, marginalize, norm=norm)
    ref_v = abs(o32["total"] - o64["total"]) / abs(o64["total"])
    ref_g = rel_linf(o32["grad"], o64["grad"])
    err_v = abs(value - o64["total"]) / abs(o64["total"])
    err_g = rel_linf(grad, o64["grad"])
    print(f"gmm16 {label} shifts={shifts} {'lse' if marginalize else 'max'}: value kernel {err_v:.2e} fp32-oracle {ref_v:.2e} | "
          f"gradient kernel {err_g:.2e} fp32-oracle {ref_g:.2e}")
    if not marginalize:
        err_l = _log_prob_error(model, flux_np, stride, shifts, o64, norm=norm)
        clear = o64["margin"] > 2.0 * err_l
        print(f"gmm16 {label}: log-prob abs error {err_l:.2e}, min margin {o64['margin'].min():.3g}, "
              f"{int((~clear).sum())} of {clear.size} patches under the margin")
        assert (~clear).mean() <= 0.01, "the inputs leave too many patches without a clear winner"
        assert np.array_equal(arg[clear], o64["arg"][clear]), "a wrong winner where the float64 margin is clear"
        assert np.array_equal(arg < 0, ~o64["keep"]), "the filtered patches differ"
    assert err_v <= max(FACTOR * ref_v, FLOOR), f"value: {err_v:.2e} > max(4 x {ref_v:.2e}, 1e-6)"
    assert err_g <= max(FACTOR * ref_g, FLOOR), f"gradient: {err_g:.2e} > max(4 x {ref_g:.2e}, 1e-6)"
    return o64


# ---------------------------------------------------------------------------------------------- 1. fixture parity
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("normed", [False, True])
def test_fixture_parity(golden, models, normed, marginalize):
    """Value and gradient of the reference's GMMPatchPrior on 16x16 patches (and the float64 oracle at the measured
    bound); the one filtered patch contributes nothing."""
    from jolideco_amd.utils.norms import ASinhImageNorm

    g = golden("gmm16")
    arrays = cases.synthetic_mixture(cases.K, cases.SEED)
    assert cases.mixture_checksum(arrays) == pytest.approx(float(g["gmm/checksum"]), rel=1e-13)
    model = models(cases.K, cases.SEED)
    norm = ASinhImageNorm(**cases.ASINH) if normed else None
    got = _run(model, g["flux"], cases.STRIDE, (0, 0), marginalize, norm=norm)
    o64 = _check_case(model, arrays, g["flux"], cases.STRIDE, (0, 0), marginalize, norm=norm, got=got,
                      label=f"fixture {'asinh' if normed else 'bare'}")
    scale = cases.prior_scale(cases.SHAPE, cases.STRIDE)
    tag = f"{'asinh' if normed else 'bare'}/{'lse' if marginalize else 'max'}"
    # against the reference's float32 numbers: its own distance from float64, plus ours
    value, grad, arg = got
    assert value * scale == pytest.approx(float(g[f"{tag}/value"]), rel=1e-5)
    assert rel_linf(grad * scale, g[f"{tag}/grad"]) < 1e-5
    if not normed:
        assert int((~o64["keep"]).sum()) == 1 and not o64["keep"][0]
        assert np.all(grad[:8, :8] == 0), "the filtered patch left a gradient on pixels only it covers"
        if not marginalize:
            assert arg[0] == -1 and np.all(arg[1:] >= 0)
        # the value is the sum over the 29 kept patches: dropping the filter would add a term of about -1e13
        assert abs(value) < 1e7


def test_fixture_log_prob_matrix(golden, models):
    from oracle import cpu_ref

    g = golden("gmm16")
    model = models(cases.K, cases.SEED)
    x = cases.mean_free_patches(cases.fixture_flux(filtered=False), cases.STRIDE)
    got = model.estimate_log_prob(torch.from_numpy(x).to(DEV)).cpu().numpy()
    with cpu_ref.precision(np.float64):
        gmm64 = cpu_ref.GMM.from_numpy(*cases.synthetic_mixture(cases.K, cases.SEED), stride=cases.STRIDE)
        ref64 = cpu_ref.gmm_log_prob(cpu_ref._tensor(x), gmm64).numpy()
    err, ref = rel_linf(got, ref64), rel_linf(g["log_prob"], ref64)
    print(f"gmm16 log-prob matrix: kernel {err:.2e} fp32-reference {ref:.2e} (rel Linf against float64)")
    assert got.shape == (30, cases.K)
    assert err <= max(FACTOR * ref, FLOOR)
    assert np.array_equal(got.argmax(axis=1), ref64.argmax(axis=1))


# ---------------------------------------------------------------------------------------------- 2. shapes and shifts
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("index", range(len(SHAPE_CASES)))
def test_shapes_and_shifts(models, index, marginalize):
    """Every shape with shifts (0, 0), (4, -4), (-3, 2): parity at the measured bound, and the shifts read from device
    memory give the bits of the by-value form."""
    shape, stride = SHAPE_CASES[index]
    arrays, model = cases.synthetic_mixture(cases.K, cases.SEED), models(cases.K, cases.SEED)
    flux = cases.case_flux(shape, 1610 + index)
    for shifts in SHIFTS:
        got = _run(model, flux, stride, shifts, marginalize)
        dev = _run(model, flux, stride, shifts, marginalize, on_device=True)
        assert got[0] == dev[0] and np.array_equal(got[1], dev[1]), "shift_dev differs from the by-value form"
        assert marginalize or np.array_equal(got[2], dev[2])
        _check_case(model, arrays, flux, stride, shifts, marginalize, got=got, label=f"{shape} stride {stride}")
        # pixels no patch covers receive nothing (un-rolled frame)
        cover = np.zeros(shape, dtype=bool)
        n_py, n_px = (shape[0] - 16) // stride + 1, (shape[1] - 16) // stride + 1
        cover[: (n_py - 1) * stride + 16, : (n_px - 1) * stride + 16] = True
        cover = np.roll(cover, (-shifts[0], -shifts[1]), axis=(0, 1))
        assert np.all(got[1][~cover] == 0) and np.any(got[1][cover] != 0)


@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("side", ["below", "at"])
def test_both_tile_sizes(models, side, marginalize):
    """The library gives a block 16 patches until 32-patch tiles would reach every compute unit, then 32 (two
    accumulators per fragment of a factor).  Every other case here is far below that threshold; these two images, 91
    patches wide, sit just below it and on it (8099 / 8190 patches on a 256-CU board)."""
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    rows = next(r for r in range(1, 4096) if (r * 91 + 31) // 32 >= n_cu) - (1 if side == "below" else 0)
    shape = (16 + 8 * (rows - 1), 16 + 8 * 90)
    assert ((cases.n_patches(shape, 8) + 31) // 32 >= n_cu) == (side == "at")
    arrays, model = cases.synthetic_mixture(3, 1623), models(3, 1623)
    _check_case(model, arrays, cases.case_flux(shape, 1690), 8, (-3, 2), marginalize, label=f"tile threshold, {side}: {shape}")


# ---------------------------------------------------------------------------------------------- 3. number of components
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("k", [1, 3, 17, 200])
def test_number_of_components(models, k, marginalize):
    arrays, model = cases.synthetic_mixture(k, 1620 + k), models(k, 1620 + k)
    flux = cases.case_flux((64, 64), 1630 + k)
    _check_case(model, arrays, flux, 8, (2, -1), marginalize, label=f"K={k}")


def test_logsumexp_with_competing_components():
    """The synthetic mixtures above have one dominant component per patch (logsumexp = max to rounding).  Here six
    components share one covariance and differ by small means and weights, so several responsibilities are of order one
    on every patch and the backward pass really sums over k.  The responsibilities exp(l_k - lse) magnify the rounding
    of l_k (of order 1e-2 absolute at |l| ~ 1e4), in the float32 oracle as in the kernel: the bound is the measured one."""
    _, cov, _ = cases.synthetic_mixture(1, 1680)
    rs = np.random.RandomState(1681)
    k = 6
    means = (0.002 * rs.normal(size=(k, 256))).astype(np.float32).astype(np.float64)
    weights = rs.dirichlet(np.ones(k) * 5).astype(np.float32).astype(np.float64)
    arrays = (means, np.repeat(cov, k, axis=0), weights)
    model, flux = _model(arrays), cases.case_flux((40, 56), 1682)
    o64 = _check_case(model, arrays, flux, 8, (1, 2), True, label="competing components")
    resp = np.exp(o64["loglike"] - o64["loglike"].max(axis=1, keepdims=True))
    resp /= resp.sum(axis=1, keepdims=True)
    assert np.median(resp.max(axis=1)) < 0.8 and (resp > 0.05).sum(axis=1).mean() > 2


@pytest.mark.parametrize("marginalize", [False, True])
def test_factors_that_are_not_triangular(marginalize):
    """Cholesky-built mixtures are upper triangular and take the kernels that skip the zero blocks.  Factors with a
    filled lower triangle (`cases.dense_factors`) take the instantiations that skip nothing -- forward, backward and
    `estimate_log_prob` (the measured log-probability error) -- at 16 patches per block whatever the size."""
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    arrays = cases.synthetic_mixture(3, 1695)
    factors = cases.dense_factors(arrays, 1696)
    assert np.abs(np.tril(factors, -1)).max() > 0
    model = GaussianMixtureModel(arrays[0], arrays[1], arrays[2], factors, meta=GaussianMixtureModelMeta(stride=cases.STRIDE))
    assert model.handle(DEV)._handle is not None
    from jolideco_amd import _hip

    assert _hip.lib().jd_gmm_is_triangular(model.handle(DEV)._handle) == 0
    flux = cases.case_flux((45, 61), 1697)
    for shifts in ((0, 0), (-3, 2)):
        o64 = cases.oracle(flux, arrays, 8, shifts, marginalize, np.float64, factors=factors)
        o32 = cases.oracle(flux, arrays, 8, shifts, marginalize, np.float32, factors=factors)
        value, grad, arg = _run(model, flux, 8, shifts, marginalize)
        ref_v, ref_g = abs(o32["total"] - o64["total"]) / abs(o64["total"]), rel_linf(o32["grad"], o64["grad"])
        err_v, err_g = abs(value - o64["total"]) / abs(o64["total"]), rel_linf(grad, o64["grad"])
        print(f"gmm16 dense factors shifts={shifts} {'lse' if marginalize else 'max'}: value kernel {err_v:.2e} fp32-oracle {ref_v:.2e} | "
              f"gradient kernel {err_g:.2e} fp32-oracle {ref_g:.2e}")
        if not marginalize:
            err_l = _log_prob_error(model, flux, 8, shifts, o64)
            clear = o64["margin"] > 2.0 * err_l
            print(f"gmm16 dense factors: log-prob abs error {err_l:.2e}, min margin {o64['margin'].min():.3g}, "
                  f"{int((~clear).sum())} of {clear.size} patches under the margin")
            assert (~clear).mean() <= 0.01 and np.array_equal(arg[clear], o64["arg"][clear])
        assert err_v <= max(FACTOR * ref_v, FLOOR), f"value: {err_v:.2e} > max(4 x {ref_v:.2e}, 1e-6)"
        assert err_g <= max(FACTOR * ref_g, FLOOR), f"gradient: {err_g:.2e} > max(4 x {ref_g:.2e}, 1e-6)"


# ---------------------------------------------------------------------------------------------- 4. paths
@pytest.mark.parametrize("marginalize", [False, True])
def test_autograd_equals_device_fwd_bwd_and_calls_repeat(models, marginalize):
    from jolideco_amd import GMMPatchPrior

    prior = GMMPatchPrior(gmm=models(cases.K, cases.SEED), marginalize=marginalize, cycle_spin=False)
    flux_np = cases.case_flux((45, 61), 1640)
    flux = torch.from_numpy(flux_np).to(DEV).reshape(1, 1, 45, 61).requires_grad_(True)
    value = prior(flux)
    value.backward()
    out = []
    for _ in range(2):
        v, g = torch.zeros(1, device=DEV), torch.zeros((45, 61), device=DEV)
        prior.device_fwd_bwd(flux.detach(), v, grad=g, coef=1.0, shifts=None)
        torch.cuda.synchronize()
        out.append((float(v), g.cpu().numpy()))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]), "two consecutive calls differ"
    assert float(value.detach()) == out[0][0] and np.array_equal(flux.grad.cpu().numpy()[0, 0], out[0][1])
    assert np.abs(out[0][1]).max() > 0
    # accumulate semantics of the device scalar and the gradient image
    v, g = torch.full((1,), 2.0, device=DEV), torch.ones((45, 61), device=DEV)
    scale = prior.log_like_weight / flux.numel()
    prior.gmm.handle(DEV).prior_fwd_bwd(flux.detach().reshape(45, 61), 8, None, v, scale, grad=g, grad_coef=scale,
                                        marginalize=marginalize, accumulate_value=True)
    torch.cuda.synchronize()
    assert float(v) == pytest.approx(2.0 + out[0][0], rel=1e-6)
    assert rel_linf(g.cpu().numpy() - 1.0, out[0][1]) < 1e-5


def test_shared_handle_alternates_between_norms(models):
    from jolideco_amd import GMMPatchPrior
    from jolideco_amd.utils.norms import ASinhImageNorm

    model = models(cases.K, cases.SEED)
    bare = GMMPatchPrior(gmm=model, cycle_spin=False)
    normed = GMMPatchPrior(gmm=model, cycle_spin=False, norm=ASinhImageNorm(**cases.ASINH))
    flux = torch.from_numpy(cases.case_flux((40, 56), 1650)).to(DEV)
    out = []
    for prior in (bare, normed, bare, normed):
        v, g = torch.zeros(1, device=DEV), torch.zeros_like(flux)
        prior.device_fwd_bwd(flux, v, grad=g, coef=1.0, shifts=(1, 2))
        torch.cuda.synchronize()
        out.append((float(v), g.cpu().numpy()))
    assert out[0][0] == out[2][0] and np.array_equal(out[0][1], out[2][1])
    assert out[1][0] == out[3][0] and np.array_equal(out[1][1], out[3][1])
    assert out[0][0] != out[1][0]


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refused_forms_return_invalid_and_the_handle_stays_usable(models):
    from jolideco_amd import _hip
    from jolideco_amd.ops import ptr, stream_ptr

    lib, model = _hip.lib(), models(cases.K, cases.SEED)
    handle = model.handle(DEV)
    flux = torch.from_numpy(cases.case_flux((40, 56), 1660)).to(DEV)
    value, grad, band = torch.zeros(1, device=DEV), torch.zeros_like(flux), torch.zeros_like(flux)
    dev, cf = torch.device(DEV), ctypes.c_float

    def fwd_bwd(rows=(0, -1), phases=3):
        return lib.jd_gmm_prior_fwd_bwd(handle._handle, ptr(flux), 40, 56, 8, 0, 0, rows[0], rows[1], 0, cf(1.0), ptr(value), 0,
                                        cf(1.0), ptr(grad), None, None, phases, stream_ptr(dev))

    for kwargs, word in (({"rows": (0, 2)}, b"shard"), ({"rows": (1, 4)}, b"shard"), ({"phases": 1}, b"phases"),
                         ({"phases": 2}, b"phases")):
        assert fwd_bwd(**kwargs) == -1
        assert b"D = 256" in lib.jd_last_error() and word in lib.jd_last_error()
    assert lib.jd_gmm_prior_band_fwd_bwd(handle._handle, ptr(flux), 40, 56, 8, 0, 0, 0, -1, 0, cf(1.0), ptr(value), 0, cf(1.0),
                                         ptr(band), stream_ptr(dev)) == -1
    assert b"D = 256" in lib.jd_last_error() and b"band" in lib.jd_last_error()
    step = _hip.Step()
    assert lib.jd_gmm_prior_fwd_bwd_step(handle._handle, ptr(flux), 40, 56, 8, 0, 0, 0, cf(1.0), ptr(value), 0, cf(1.0),
                                         ctypes.byref(step), None, 3, stream_ptr(dev)) == -1
    assert b"D = 256" in lib.jd_last_error() and b"step" in lib.jd_last_error()
    torch.cuda.synchronize()
    assert float(value) == 0.0 and not grad.any() and not band.any(), "a refused call ran a kernel"
    # the explicit whole range is the whole image, and the next valid call works
    assert fwd_bwd(rows=(0, 4)) == 0
    torch.cuda.synchronize()
    whole = (float(value), grad.cpu().numpy().copy())
    grad.zero_()
    assert fwd_bwd() == 0
    torch.cuda.synchronize()
    assert whole[0] == float(value) and np.array_equal(whole[1], grad.cpu().numpy()) and whole[0] != 0.0


# ---------------------------------------------------------------------------------------------- 6. fits
def _fit_inputs(golden):
    from jolideco_amd import GMMPatchPrior, SpatialFluxComponent

    g = golden("gmm16")
    arrays = cases.synthetic_mixture(cases.FIT_K, cases.FIT_GMM_SEED)
    assert cases.mixture_checksum(arrays) == pytest.approx(float(g["fit/gmm/checksum"]), rel=1e-13)
    comp = SpatialFluxComponent.from_numpy(flux=g["fit/flux_init"], prior=GMMPatchPrior(gmm=_model(arrays)))
    return g, unpack_datasets(g, "fit/data/"), comp


def test_fit_matches_the_reference(golden):
    """6 sequential epochs, 48 x 48, cycle-spin on with the default generator: final flux and trace of the reference at
    the tolerances tests/test_gpu_fit.py holds its reference-generated fits to."""
    from jolideco_amd import MAPDeconvolver

    g, datasets, comp = _fit_inputs(golden)
    res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).run(datasets, components=comp)
    err = rel_linf(res.flux_total, g["fit/flux_final"])
    print("gmm16 fit rel Linf", err)
    assert err < 1e-5
    for key, ref in g.items():
        if key.startswith("fit/trace/"):
            name = key[len("fit/trace/"):]
            np.testing.assert_allclose(res.trace_loss[name], ref, rtol=2e-5, atol=1e-6, err_msg=name)


def test_replayed_epochs_equal_the_by_value_epochs(golden, monkeypatch):
    """Planned epochs read the shifts from device memory; captured and replayed (JOLIDECO_GRAPH=1) they give the bits of
    the by-value epochs, and the reference's flux."""
    from jolideco_amd import MAPDeconvolver

    out = {}
    for mode in ("host", "graph"):
        monkeypatch.setenv("JOLIDECO_STEP_SCALARS", "host" if mode == "host" else "device")
        monkeypatch.setenv("JOLIDECO_GRAPH", "1" if mode == "graph" else "0")
        g, datasets, comp = _fit_inputs(golden)
        session = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).session(datasets, components=comp)
        for _ in range(cases.FIT_EPOCHS):
            session.epoch()
        torch.cuda.synchronize()
        out[mode] = (session.states[0].flux_cur.cpu().numpy().copy(), len(session._graphs))
    assert out["host"][1] == 0 and out["graph"][1] >= 1, "no epoch was captured"
    assert np.array_equal(out["graph"][0], out["host"][0])
    assert rel_linf(out["graph"][0].reshape(cases.FIT_SHAPE), g["fit/flux_final"]) < 1e-5


def test_two_components_with_an_8x8_and_a_16x16_prior(models):
    """One fit, two flux components, an 8x8 and a 16x16 GMM prior (each with its own default-seeded generator) against
    `cpu_ref.map_fit_sequential`."""
    from jolideco_amd import FluxComponents, GMMPatchPrior, MAPDeconvolver, SpatialFluxComponent
    from jolideco_amd.data import point_source_gauss_psf
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
    from oracle import cpu_ref

    rs = np.random.RandomState(1670)
    datasets = {f"o{i}": point_source_gauss_psf(shape=(48, 40), sigma_psf=2 + i, random_state=rs) for i in range(2)}
    for d in datasets.values():
        d.pop("flux")
    inits = {"fine": rs.gamma(30, size=(48, 40)), "coarse": rs.gamma(30, size=(48, 40))}
    a8 = cpu_ref.synthetic_gmm(4, 64, seed=2)
    a16 = cases.synthetic_mixture(3, 1671)
    comps = FluxComponents()
    comps["fine"] = SpatialFluxComponent.from_numpy(flux=inits["fine"], prior=GMMPatchPrior(
        gmm=GaussianMixtureModel.from_numpy(*a8, meta=GaussianMixtureModelMeta(stride=4)), generator=torch.Generator(device="cpu")))
    comps["coarse"] = SpatialFluxComponent.from_numpy(flux=inits["coarse"], prior=GMMPatchPrior(
        gmm=models(3, 1671), generator=torch.Generator(device="cpu")))
    res = MAPDeconvolver(n_epochs=4, display_progress=False, device=DEV).run(datasets, components=comps)
    priors = {"fine": cpu_ref.GMMPatchPriorRef(cpu_ref.GMM.from_numpy(*a8, stride=4), generator=torch.Generator(device="cpu")),
              "coarse": cpu_ref.GMMPatchPriorRef(cpu_ref.GMM.from_numpy(*a16, stride=8), generator=torch.Generator(device="cpu"))}
    final, trace = cpu_ref.map_fit_sequential(datasets, inits, priors, n_epochs=4)
    fl = res.components.to_numpy()
    for name in ("fine", "coarse"):
        err = rel_linf(fl[name], final[name])
        print("gmm16 two components", name, err)
        assert err < 1e-5
    assert abs(res.trace_loss[-1]["total"] - trace[-1]["total"]) < 1e-4 * abs(trace[-1]["total"])

"""GPU: `MultiScalePrior` (jolideco_amd/csrc/multiscale.hip + the inner prior's kernels) against the float64 evaluations of
tests/multiscale_cases.py and tests/golden/multiscale.npz (written from the live reference by
tools/make_golden_multiscale.py).

Tolerances are measured, not chosen (the rule of tests/test_gpu_gmm16.py): the device's relative L-infinity error against
float64 may be at most 4 times the error of the SAME formula evaluated in float32 on the CPU against float64, with a floor
of 1e-6 -- value and gradient separately.  In max mode a near tie between two components would flip an arg-max: the seeds
of the cases leave, over every patch of every level of every case, a float64 margin (best minus runner-up) of at least
twice the device's measured log-probability error, which is asserted.  Figures measured on an MI355X:
profiles/multiscale/README.md."""
import numpy as np
import pytest
import torch

import multiscale_cases as cases
from conftest import rel_linf, unpack_datasets
from jolideco_amd import MultiScalePrior  # noqa: F401  (every test of this file is about it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 4.0, 1e-6


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bound(e32):
    return max(FACTOR * e32, FLOOR)


# ------------------------------------------------------------------------------------------------ 1. the two kernels alone
def _down(x, f, taps, shifts=None, keep_g=True):
    from jolideco_amd.ops import multiscale_down

    H, W = x.shape
    g = torch.full((H, W), np.nan, device=DEV) if keep_g else None
    d = torch.full((H // f, W // f), np.nan, device=DEV)
    dd = torch.full((H // f, W // f), np.nan, device=DEV)
    multiscale_down(_dev(x), f, taps, d, g_out=g, dd_zero=dd, shifts=shifts)
    torch.cuda.synchronize()
    assert bool(torch.all(dd == 0)), "dd was not zeroed"
    return (None if g is None else g.cpu().numpy()), d.cpu().numpy()


def _up(dd, dg, shape, f, taps, out=None, shifts=None, rolled=False):
    from jolideco_amd.ops import multiscale_up_adjoint

    out = torch.full(shape, np.nan, device=DEV) if out is None else out
    multiscale_up_adjoint(_dev(dd), f, taps, out, dg=None if dg is None else _dev(dg), shifts=shifts, rolled=rolled)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("index", range(len(cases.KERNEL_CASES)))
def test_down_against_float64(index):
    shape, f, n_taps = cases.KERNEL_CASES[index]
    taps = cases.kernel_taps(n_taps, 4500 + index)
    x = np.random.RandomState(4510 + index).gamma(20, size=shape).astype(np.float32)
    g, d = _down(x, f, taps)
    g64, d64 = cases.down_numpy(x, f, taps)
    g32, d32 = cases.down_numpy(x, f, taps, dtype=np.float32)
    for name, got, r64, r32 in (("g", g, g64, g32), ("d", d, d64, d32)):
        err, e32 = rel_linf(got, r64), rel_linf(r32, r64)
        print(f"multiscale down {shape} f={f} taps={n_taps} {name}: kernel {err:.2e} float32-numpy {e32:.2e}")
        assert err <= _bound(e32), f"{name}: {err:.2e} > max(4 x {e32:.2e}, 1e-6)"
    assert d.shape == (shape[0] // f, shape[1] // f)
    _, d_only = _down(x, f, taps, keep_g=False)  # (the last level: g is not stored)
    assert np.array_equal(d_only, d)


@pytest.mark.parametrize("index", range(len(cases.KERNEL_CASES)))
def test_up_adjoint_against_float64_and_by_the_inner_product(index):
    """`up` against float64, with and without dg; and <down(x), y> = <x, up(y)> with the device's own outputs.  The bound
    of the identity: each side is a sum of products with an exact operand, so it is off by at most (relative L-infinity
    error of the computed operand) x max|operand| x sum|exact operand|; the computed operands are allowed 4 x their
    float32-numpy error (floor 1e-6), as above."""
    shape, f, n_taps = cases.KERNEL_CASES[index]
    taps = cases.kernel_taps(n_taps, 4500 + index)
    rs = np.random.RandomState(4520 + index)
    x = rs.gamma(20, size=shape).astype(np.float32)
    yd = rs.normal(size=(shape[0] // f, shape[1] // f)).astype(np.float32)
    yg = rs.normal(size=shape).astype(np.float32)
    bounds = {}
    for label, dg in (("with dg", yg), ("last level", None)):
        got = _up(yd, dg, shape, f, taps)
        u64, u32 = cases.up_numpy(yd, dg, shape, f, taps), cases.up_numpy(yd, dg, shape, f, taps, dtype=np.float32)
        err, e32 = rel_linf(got, u64), rel_linf(u32, u64)
        print(f"multiscale up {shape} f={f} taps={n_taps} {label}: kernel {err:.2e} float32-numpy {e32:.2e}")
        assert err <= _bound(e32), f"{label}: {err:.2e} > max(4 x {e32:.2e}, 1e-6)"
        bounds[label] = (got, _bound(e32) * np.abs(u64).max())
    g, d = _down(x, f, taps)
    g64, d64 = cases.down_numpy(x, f, taps)
    g32, d32 = cases.down_numpy(x, f, taps, dtype=np.float32)
    as64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    lhs = np.sum(as64(g) * as64(yg)) + np.sum(as64(d) * as64(yd))
    rhs = np.sum(as64(x) * as64(bounds["with dg"][0]))
    slack = (_bound(rel_linf(g32, g64)) * np.abs(g64).max() * np.abs(yg).sum() + _bound(rel_linf(d32, d64)) * np.abs(d64).max() * np.abs(yd).sum()
             + bounds["with dg"][1] * np.abs(x).sum())
    print(f"multiscale inner product {shape} f={f}: <down x, y> = {lhs:.9g}, <x, up y> = {rhs:.9g}, |difference| {abs(lhs - rhs):.3g} "
          f"(bound {slack:.3g})")
    assert abs(lhs - rhs) <= slack


def test_rolled_first_level_and_its_inverse():
    """33 x 41: the loads of `down` read the rolled image; `up` with rolled=1 ADDS its result at the un-rolled pixel."""
    shape, f, taps = (33, 41), 2, cases.kernel_taps(7, 4530)
    rs = np.random.RandomState(4531)
    x = rs.gamma(20, size=shape).astype(np.float32)
    for shifts in ((2, -1), (-2, 2), (0, 0), (35, -43)):
        g, d = _down(x, f, taps, shifts=shifts)
        g64, d64 = cases.down_numpy(x, f, taps, shifts=shifts)
        g32, d32 = cases.down_numpy(x, f, taps, shifts=shifts, dtype=np.float32)
        assert rel_linf(g, g64) <= _bound(rel_linf(g32, g64)) and rel_linf(d, d64) <= _bound(rel_linf(d32, d64)), shifts
        # the roll only moves pixels: the device's un-rolled run on the rolled image gives the same bits
        g0, d0 = _down(np.roll(x, shifts, axis=(0, 1)), f, taps)
        assert np.array_equal(g0, g) and np.array_equal(d0, d), shifts
        yd = rs.normal(size=d.shape).astype(np.float32)
        yg = rs.normal(size=shape).astype(np.float32)
        base = rs.normal(size=shape).astype(np.float32)
        plain = _up(yd, yg, shape, f, taps)
        rolled = _up(yd, yg, shape, f, taps, out=_dev(base), shifts=shifts, rolled=True)
        expected = base + np.roll(plain, (-shifts[0], -shifts[1]), axis=(0, 1))  # (one float32 addition per pixel)
        assert np.array_equal(rolled, expected), shifts


# ------------------------------------------------------------------------------------------------ 2. the prior on every case
def _model(case):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    return GaussianMixtureModel.from_numpy(*cases.case_mixture(case), meta=GaussianMixtureModelMeta(stride=case["stride"]))


@pytest.fixture(scope="module")
def priors():
    """name -> (MultiScalePrior, model) of a case, built once: the inner generator is seeded like the case's draws"""
    from jolideco_amd import GMMPatchPrior, MultiScalePrior

    cache = {}

    def get(name):
        case = cases.CASES[name]
        if name not in cache:
            model = _model(case)
            inner = GMMPatchPrior(gmm=model, cycle_spin=case["inner_spin"], marginalize=case["marginalize"],
                                  norm=cases.make_norm(case), generator=torch.Generator(device="cpu"))
            cache[name] = (MultiScalePrior(inner, n_levels=case["n_levels"], weights=case["weights"], cycle_spin=case["outer_spin"],
                                           anti_alias=case["anti_alias"]), model)
        prior, model = cache[name]
        if case["inner_seed"] is not None:
            prior.prior.generator.manual_seed(case["inner_seed"])
        return prior, model

    return get


def _check(name, value, grad, label):
    o32, o64 = cases.cached_restate(name, "float32"), cases.cached_restate(name, "float64")
    ref_v, ref_g = abs(o32["value"] - o64["value"]) / abs(o64["value"]), rel_linf(o32["grad"], o64["grad"])
    err_v, err_g = abs(value - o64["value"]) / abs(o64["value"]), rel_linf(grad, o64["grad"])
    print(f"multiscale {name} {label}: value kernel {err_v:.2e} float32-restatement {ref_v:.2e} | gradient kernel {err_g:.2e} "
          f"float32-restatement {ref_g:.2e}")
    assert err_v <= _bound(ref_v), f"value: {err_v:.2e} > max(4 x {ref_v:.2e}, 1e-6)"
    assert err_g <= _bound(ref_g), f"gradient: {err_g:.2e} > max(4 x {ref_g:.2e}, 1e-6)"


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_fwd_bwd(priors, name):
    """Value and gradient through the fused path, against the float64 restatement; the gradient is ACCUMULATED with the
    coefficient; a forward-only call gives the value; two evaluations give identical bits."""
    case = cases.CASES[name]
    prior, _ = priors(name)
    flux = _dev(cases.case_flux(case))[None, None]
    shifts = cases.draws(case)
    runs = []
    for _ in range(2):
        value, grad = torch.full((1,), np.nan, device=DEV), torch.zeros(case["shape"], device=DEV)
        prior.device_fwd_bwd(flux, value, grad=grad, coef=1.0, shifts=shifts)
        torch.cuda.synchronize()
        runs.append((float(value), grad.cpu().numpy()))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]), "two evaluations differ"
    _check(name, runs[0][0], runs[0][1], "device_fwd_bwd")
    forward = torch.full((1,), np.nan, device=DEV)
    prior.device_fwd_bwd(flux, forward, shifts=shifts)  # (the inner prior may sum a forward-only pass in another order)
    _check(name, float(forward), runs[0][1], "forward only")
    base = np.random.RandomState(4540).normal(size=case["shape"]).astype(np.float32)
    acc, value = _dev(base), torch.zeros(1, device=DEV)
    prior.device_fwd_bwd(flux, value, grad=acc, coef=-0.5, shifts=shifts)
    o64 = cases.cached_restate(name, "float64")
    assert float(value) == runs[0][0]
    scale = np.abs(o64["grad"]).max() * 0.5
    o32 = cases.cached_restate(name, "float32")
    assert np.abs(acc.cpu().numpy() - base - (-0.5) * o64["grad"]).max() <= _bound(rel_linf(o32["grad"], o64["grad"])) * scale + 2.0**-23 * np.abs(base).max()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_call_is_the_autograd_seam(priors, name):
    """`prior(flux)` draws once from the inner prior's generator (the case's draws) and back-propagates."""
    case = cases.CASES[name]
    prior, _ = priors(name)
    flux = _dev(cases.case_flux(case))[None, None].requires_grad_(True)
    value = prior(flux)
    (2.0 * value).backward()
    torch.cuda.synchronize()
    assert prior.last_shifts == cases.draws(case)
    assert value.shape == () and flux.grad.shape == flux.shape
    _check(name, float(value.detach()), flux.grad.cpu().numpy()[0, 0] / 2.0, "__call__")
    if case["inner_seed"] is not None:
        prior.prior.generator.manual_seed(case["inner_seed"])
    with torch.no_grad():
        _check(name, float(prior(flux.detach())), flux.grad.cpu().numpy()[0, 0] / 2.0, "__call__ without a gradient")


def test_reference_numbers(golden, priors):
    """Against the reference's own float32 numbers (outer cycle spin off): its distance from float64, plus ours."""
    g = golden("multiscale")
    for name in cases.REFERENCE_CASES:
        case = cases.CASES[name]
        prior, _ = priors(name)
        value, grad = torch.zeros(1, device=DEV), torch.zeros(case["shape"], device=DEV)
        prior.device_fwd_bwd(_dev(g[f"{name}/flux"])[None, None], value, grad=grad, coef=1.0, shifts=cases.draws(case))
        o32, o64 = cases.cached_restate(name, "float32"), cases.cached_restate(name, "float64")
        ref_v = abs(float(g[f"{name}/value"]) - o64["value"]) / abs(o64["value"])
        ref_g = rel_linf(g[f"{name}/grad"], o64["grad"])
        own_v = _bound(abs(o32["value"] - o64["value"]) / abs(o64["value"]))
        own_g = _bound(rel_linf(o32["grad"], o64["grad"]))
        assert abs(float(value) - float(g[f"{name}/value"])) <= (ref_v + own_v) * abs(o64["value"]), name
        assert np.abs(grad.cpu().numpy() - g[f"{name}/grad"]).max() <= (ref_g + own_g) * np.abs(o64["grad"]).max(), name


def test_argmax_margins_are_clear(golden, priors):
    """Over every patch of every level of every max-mode case the float64 margin between the best and the second component
    is at least twice the device's measured log-probability error (so no arg-max can flip); no patch is left out."""
    g = golden("multiscale")
    worst_margin, worst_error = np.inf, 0.0
    for name, case in cases.CASES.items():
        if case["marginalize"]:
            continue
        _, model = priors(name)
        shifts = cases.draws(case)
        o64 = cases.cached_restate(name, "float64")
        margin = cases.margins(o64["levels"])
        assert margin.min() == pytest.approx(float(g[f"{name}/min_margin"]), rel=1e-6)
        p = int(round(case["D"] ** 0.5))
        error = 0.0
        for level in o64["levels"]:
            x = cases.mean_free_patches(level["image"], p, case["stride"], shifts[1 + level["level"]])
            assert x.shape[0] == level["loglike"].shape[0]
            got = model.estimate_log_prob(_dev(x)).cpu().numpy().astype(np.float64)
            error = max(error, float(np.abs(got - level["loglike"]).max()))
        print(f"multiscale {name}: {margin.size} patches, min margin {margin.min():.3g}, log-probability abs error {error:.2e}")
        assert margin.min() >= 2.0 * error, name
        worst_margin, worst_error = min(worst_margin, margin.min()), max(worst_error, error)
    print(f"multiscale margins: smallest {worst_margin:.3g}, largest log-probability error {worst_error:.2e}")


def test_no_allocation_and_no_synchronisation_after_the_first_call(priors):
    """The work buffers belong to the prior, per device and shape: a second call allocates nothing (the allocator's
    counters stand still) and the buffers are the same tensors."""
    name = "33x41-L3"
    case = cases.CASES[name]
    prior, _ = priors(name)
    flux = _dev(cases.case_flux(case))[None, None]
    value, grad = torch.zeros(1, device=DEV), torch.zeros(case["shape"], device=DEV)
    shifts = cases.draws(case)
    prior.device_fwd_bwd(flux, value, grad=grad, coef=1.0, shifts=shifts)
    torch.cuda.synchronize()
    work = prior._buffers_for(flux)
    pointers = [t.data_ptr() for t in work["full"] + work["d"] + work["dd"]] + [work["values"].data_ptr()]
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    prior.device_fwd_bwd(flux, value, grad=grad, coef=1.0, shifts=shifts)
    prior.device_fwd_bwd(flux, value, shifts=shifts)
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    work = prior._buffers_for(flux)
    assert pointers == [t.data_ptr() for t in work["full"] + work["d"] + work["dd"]] + [work["values"].data_ptr()]


# ------------------------------------------------------------------------------------------------ 3. fits
def _fit_component():
    from jolideco_amd import GMMPatchPrior, MultiScalePrior, SpatialFluxComponent
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    datasets, flux_init, arrays = cases.fit_inputs()
    fit = cases.FIT
    gmm = GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=fit["stride"]))
    prior = MultiScalePrior(GMMPatchPrior(gmm=gmm), n_levels=fit["n_levels"], cycle_spin=False)
    return datasets, SpatialFluxComponent.from_numpy(flux=flux_init, prior=prior)


def test_fit_matches_the_reference(golden):
    """6 sequential epochs on 32 x 32, `MultiScalePrior(n_levels=2, cycle_spin=False)`, the inner prior cycle-spinning with
    the default generator: final flux and trace of the reference's own run (its level weights frozen)."""
    from jolideco_amd import MAPDeconvolver

    g = golden("multiscale")
    datasets, comp = _fit_component()
    stored = unpack_datasets(g, prefix="fit/data/")
    assert all(np.array_equal(stored[n][k], datasets[n][k]) for n in datasets for k in datasets[n])
    res = MAPDeconvolver(n_epochs=cases.FIT["n_epochs"], display_progress=False, device=DEV).run(datasets, components=comp)
    err = rel_linf(res.flux_total, g["fit/flux_final"])
    print("multiscale fit rel Linf", err)
    assert err < 1e-5
    for key, ref in g.items():
        if key.startswith("fit/trace/"):
            name = key[len("fit/trace/"):]
            np.testing.assert_allclose(res.trace_loss[name], ref, rtol=2e-5, atol=1e-6, err_msg=name)


def test_session_runs_by_value_and_captures_nothing(golden, monkeypatch):
    monkeypatch.setenv("JOLIDECO_GRAPH", "1")
    from jolideco_amd import MAPDeconvolver

    datasets, comp = _fit_component()
    session = MAPDeconvolver(n_epochs=cases.FIT["n_epochs"], display_progress=False, device=DEV).session(datasets, components=comp)
    assert session._planned_capable() is False
    for _ in range(cases.FIT["n_epochs"]):
        session.epoch()
    torch.cuda.synchronize()
    assert session._graphs == {} and session.step_scalars is None
    flux = session.states[0].flux_cur.cpu().numpy().reshape(cases.FIT["shape"])
    assert rel_linf(flux, golden("multiscale")["fit/flux_final"]) < 1e-5


@pytest.mark.parametrize("fit_mode", ["sequential", "joint"])
def test_two_components_with_a_plain_and_a_multiscale_prior(fit_mode):
    """One fit, a plain GMM prior on one component and a `MultiScalePrior` on the other (each inner prior with its own
    default-seeded generator), against `cpu_ref` over the restatement."""
    from jolideco_amd import FluxComponents, GMMPatchPrior, MAPDeconvolver, MultiScalePrior, SpatialFluxComponent
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
    from oracle import cpu_ref

    datasets, _, arrays = cases.fit_inputs()
    rs = np.random.RandomState(4550)
    inits = {"fine": rs.gamma(30, size=cases.FIT["shape"]), "coarse": rs.gamma(30, size=cases.FIT["shape"])}
    plain = cases.synthetic_mixture(4, 64, 4104)
    model = lambda a: GaussianMixtureModel.from_numpy(*a, meta=GaussianMixtureModelMeta(stride=4))  # noqa: E731
    comps = FluxComponents()
    comps["fine"] = SpatialFluxComponent.from_numpy(flux=inits["fine"], prior=GMMPatchPrior(
        gmm=model(plain), generator=torch.Generator(device="cpu")))
    comps["coarse"] = SpatialFluxComponent.from_numpy(flux=inits["coarse"], prior=MultiScalePrior(
        GMMPatchPrior(gmm=model(arrays), generator=torch.Generator(device="cpu")), n_levels=2, cycle_spin=True))
    res = MAPDeconvolver(n_epochs=4, display_progress=False, device=DEV, fit_mode=fit_mode).run(datasets, components=comps)
    refs = {"fine": cpu_ref.GMMPatchPriorRef(cpu_ref.GMM.from_numpy(*plain, stride=4), generator=torch.Generator(device="cpu")),
            "coarse": cases.MultiScalePriorRef(cpu_ref.GMM.from_numpy(*arrays, stride=4), 4, 2, outer_spin=True,
                                               generator=torch.Generator(device="cpu"))}
    fit = cpu_ref.map_fit_sequential if fit_mode == "sequential" else cpu_ref.map_fit_joint
    final, trace = fit(datasets, inits, refs, n_epochs=4)[:2]
    fl = res.components.to_numpy()
    for name in ("fine", "coarse"):
        err = rel_linf(fl[name], final[name])
        print("multiscale two components", fit_mode, name, err)
        assert err < 1e-5
    assert abs(res.trace_loss[-1]["total"] - trace[-1]["total"]) < 1e-4 * abs(trace[-1]["total"])

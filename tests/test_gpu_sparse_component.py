"""GPU: the sparse point-source flux component -- jd_sparse_render / jd_sparse_backward against the float64 oracle of
tests/sparse_cases.py (pinned against the live reference when tools/make_golden_sparse.py generated
tests/golden/sparse_component.npz), and fits with a sparse member against the fixture and the CPU fit harness.

Bound of the kernel tests, the project's rule: the error against float64 is at most 4 x the float32 CPU oracle's own error
against float64, floor 1e-6 (relative L-infinity, every gradient vector relative to its own largest magnitude).  The source
fluxes and positions of a fit: at most 4 x the float32 harness run's error against the float64 harness run, floor 1e-5; its
diffuse flux and trace: the project's fit tolerances (1e-5 relative L-infinity, rtol 1e-4).  Every case prints its figures.

Axes: ``x_pos`` runs along the rows (as in the reference); the kernels take the column coordinate first."""
import functools

import numpy as np
import pytest
import torch

import sparse_cases as cases
from conftest import GOLDEN, rel_linf, unpack_datasets
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(array):
    return torch.tensor(np.ascontiguousarray(array, dtype=np.float32), device=DEV)


def _vectors(kind, shape, use_log_flux):
    """Device vectors in the kernels' order: parameter, column coordinate (y_pos), row coordinate (x_pos)."""
    flux, x_pos, y_pos = cases.source_set(kind, shape)
    return _dev(cases.parameter(flux, use_log_flux)), _dev(y_pos), _dev(x_pos)


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("use_log_flux", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("kind", cases.SOURCE_SETS)
@pytest.mark.parametrize("shape", cases.RENDER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_render_against_float64(shape, kind, use_log_flux):
    from jolideco_amd.ops import sparse_render

    image64, _ = cases.cached_oracle(kind, shape, use_log_flux, "float64")
    image32, _ = cases.cached_oracle(kind, shape, use_log_flux, "float32")
    own = rel_linf(image32, image64)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)  # every pixel must be written
    sparse_render(*_vectors(kind, shape, use_log_flux), use_log_flux, out)
    got = out.cpu().numpy()
    err = rel_linf(got, image64)
    print(f"render {shape} {kind} {'log' if use_log_flux else 'linear'}: err {err:.2e} (float32 oracle {own:.2e})")
    assert np.all(np.isfinite(got))
    assert err <= cases.bound(own), (err, own)
    assert np.all(got[image64 == 0] == 0), "a pixel no source touches is not exactly 0"
    assert np.array_equal(got == 0, image64 == 0)


@pytest.mark.parametrize("use_log_flux", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("kind", cases.SOURCE_SETS)
@pytest.mark.parametrize("shape", cases.RENDER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward_against_float64_autograd(shape, kind, use_log_flux):
    from jolideco_amd.ops import sparse_backward

    _, grads64 = cases.cached_oracle(kind, shape, use_log_flux, "float64")
    _, grads32 = cases.cached_oracle(kind, shape, use_log_flux, "float32")
    param, cols, rows = _vectors(kind, shape, use_log_flux)
    g_param, g_cols, g_rows = (torch.full_like(param, float("nan")) for _ in range(3))  # assigned, not accumulated
    sparse_backward(param, cols, rows, use_log_flux, _dev(cases.upstream(shape)), g_param, g_cols, g_rows)
    got = [g.cpu().numpy() for g in (g_param, g_rows, g_cols)]  # (param, x_pos, y_pos)
    for name, g, g32, g64 in zip(("param", "x_pos", "y_pos"), got, grads32, grads64):
        assert np.all(np.isfinite(g)), name
        if not np.any(g64):
            assert not np.any(g), name
            continue
        own, err = rel_linf(g32, g64), rel_linf(g, g64)
        print(f"backward {shape} {kind} {'log' if use_log_flux else 'linear'} d/d{name}: err {err:.2e} (float32 oracle {own:.2e})")
        assert err <= cases.bound(own), (name, err, own)
    if kind == "b":
        # source 4 sits on exactly integer coordinates, source 6 wholly outside the image
        assert got[1][4] == 0 and got[2][4] == 0 and grads64[1][4] == 0 and grads64[2][4] == 0
        assert all(g[6] == 0 for g in got)
    if kind == "random":
        _, x_pos, y_pos = cases.source_set(kind, shape)
        outside = (x_pos <= -1) | (x_pos >= shape[0]) | (y_pos <= -1) | (y_pos >= shape[1])
        assert outside.any() and all(not np.any(g[outside]) for g in got)


@pytest.mark.parametrize("shape", [(33, 65), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_clustered_render_is_reproducible(shape):
    """A thousand sources on 64 pixels: two runs give equal bits (no atomics, index-ordered sums)."""
    from jolideco_amd.ops import sparse_render

    vectors = _vectors("clustered", shape, True)
    runs = []
    for fill in (float("nan"), 7.0):
        out = torch.full(shape, fill, dtype=torch.float32, device=DEV)
        runs.append(sparse_render(*vectors, True, out))
    assert torch.equal(runs[0], runs[1])
    touched = int((runs[0] != 0).sum())
    assert 49 <= touched <= 64, touched


def test_fixture_images_and_gradients(golden):
    """Sets (a) and (b) as the reference rendered and differentiated them."""
    from jolideco_amd.ops import sparse_backward, sparse_render

    g = golden("sparse_component")
    for tag in ("a", "b"):
        shape = tuple(int(v) for v in g[f"{tag}/shape"])
        for use_log_flux in (True, False):
            key = f"{tag}/{'log' if use_log_flux else 'linear'}"
            param, cols, rows = _dev(cases.parameter(g[f"{tag}/flux"], use_log_flux)), _dev(g[f"{tag}/y_pos"]), _dev(g[f"{tag}/x_pos"])
            image = sparse_render(param, cols, rows, use_log_flux, torch.empty(shape, dtype=torch.float32, device=DEV))
            assert rel_linf(image.cpu().numpy(), g[f"{key}/image"]) < 1e-6
            grads = [torch.empty_like(param) for _ in range(3)]
            sparse_backward(param, cols, rows, use_log_flux, _dev(cases.upstream(shape)), *grads)
            for name, grad in zip(("grad_param", "grad_y", "grad_x"), grads):
                assert rel_linf(grad.cpu().numpy(), g[f"{key}/{name}"]) < 1e-6, (key, name)


def test_autograd_seam_and_flux_components(golden):
    """`component.flux.sum().backward()` fills the three `.grad`s with the oracle's values; `FluxComponents` serves the
    rendered image beside a dense member."""
    import jolideco_amd as jd

    shape = cases.CASE_B_SHAPE
    flux, x_pos, y_pos = cases.case_b()
    comp = jd.SparseSpatialFluxComponent.from_numpy(flux=flux, x_pos=x_pos, y_pos=y_pos, shape=shape).to(DEV)
    image = comp.flux
    assert image.shape == (1, 1) + shape and image.requires_grad
    image.sum().backward()
    param = cases.parameter(flux)
    image64, grads64 = cases.oracle(param, x_pos, y_pos, shape, True, np.ones(shape), dtype=np.float64)
    image32, grads32 = cases.oracle(param, x_pos, y_pos, shape, True, np.ones(shape), dtype=np.float32)
    assert rel_linf(image.detach().cpu().numpy()[0, 0], image64) <= cases.bound(rel_linf(image32, image64))
    for p, g32, g64 in zip((comp._flux, comp.x_pos, comp.y_pos), grads32, grads64):
        if not np.any(g64):  # (a uniform upstream image: every row coordinate's taps cancel)
            assert not np.any(p.grad.cpu().numpy())
            continue
        assert rel_linf(p.grad.cpu().numpy(), g64) <= cases.bound(rel_linf(g32, g64))
    assert comp.x_pos.grad[4] == 0 and comp.y_pos.grad[4] == 0
    np.testing.assert_array_equal(comp.flux_numpy, comp.flux_upsampled.detach().cpu().numpy()[0, 0])

    diffuse = np.random.RandomState(1).gamma(2.0, size=shape).astype(np.float32)
    comps = jd.FluxComponents({"diffuse": jd.SpatialFluxComponent.from_numpy(flux=diffuse), "points": comp}).to(DEV)
    fluxes = comps.to_flux_tuple()
    assert len(fluxes) == 2 and all(f.shape == (1, 1) + shape for f in fluxes)
    assert set(comps.fluxes_numpy) == {"diffuse", "points"}
    np.testing.assert_array_equal(comps.fluxes_numpy["points"], comp.flux_numpy)
    np.testing.assert_allclose(comps.flux_total_numpy, diffuse + comp.flux_numpy, rtol=1e-6)
    np.testing.assert_allclose(comps.flux_upsampled_total_numpy, comps.flux_total_numpy, rtol=1e-6)
    assert len(comps.parameters()) == 4 and all(p.is_cuda for p in comps.parameters())


# ---------------------------------------------------------------------------------------------------- fits
def _scene(golden):
    g = golden("sparse_component")
    datasets = unpack_datasets(g, prefix="fit/data/")
    sources = tuple(g[f"fit/start/{k}"] for k in ("flux", "x_pos", "y_pos"))
    return g, datasets, g["fit/flux_init"], sources


@functools.lru_cache(maxsize=None)
def _harness(mode, use_log_flux=True, optimizer="adam", n_epochs=cases.FIT_EPOCHS):
    """The fit harness on the fixture's scene in float32 and in float64 (computed once per form)."""
    g = dict(np.load(GOLDEN / "sparse_component.npz"))
    datasets = unpack_datasets(g, prefix="fit/data/")
    sources = tuple(g[f"fit/start/{k}"] for k in ("flux", "x_pos", "y_pos"))
    kwargs = dict(mode=mode, use_log_flux=use_log_flux, optimizer=optimizer)
    run32 = cases.fit_harness(datasets, g["fit/flux_init"], sources, n_epochs, **kwargs)
    with cpu_ref.precision(np.float64):
        run64 = cases.fit_harness(datasets, g["fit/flux_init"], sources, n_epochs, **kwargs)
    return run32, run64


def _components(flux_init, sources, use_log_flux=True, frozen=False, prior_diffuse=None, prior_points=None):
    import jolideco_amd as jd

    comps = jd.FluxComponents()
    comps["diffuse"] = jd.SpatialFluxComponent.from_numpy(flux=flux_init, prior=prior_diffuse)
    comps["points"] = jd.SparseSpatialFluxComponent.from_numpy(
        flux=sources[0], x_pos=sources[1], y_pos=sources[2], shape=cases.FIT_SHAPE, use_log_flux=use_log_flux, frozen=frozen,
        prior=prior_points)
    return comps


def _check_points(tag, points, run32, run64):
    """Fluxes and positions of the fitted sparse component against the float64 harness run, each within its own bound."""
    bounds = cases.fit_bounds(run32, run64)
    got = {"flux": points.to_dict()["flux"], "x_pos": points.x_pos_numpy, "y_pos": points.y_pos_numpy}
    errors = {key: rel_linf(got[key], run64[key]) for key in got}
    print(f"{tag}: " + ", ".join(f"{key} err {errors[key]:.2e} (bound {bounds[key]:.2e})" for key in got))
    for key in got:
        assert errors[key] <= bounds[key], (key, errors[key], bounds[key])
    return errors


def test_sequential_fit_matches_the_fixture(golden):
    """Fixture (c): the reference's own fit of a diffuse component and three sources."""
    import jolideco_amd as jd

    g, datasets, flux_init, sources = _scene(golden)
    comps = _components(flux_init, sources)
    res = jd.MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).run(datasets, components=comps)
    diffuse, points = res.components["diffuse"], res.components["points"]
    err = rel_linf(diffuse.flux_upsampled_numpy, g["fit/diffuse"])
    print(f"sequential fit: diffuse flux rel Linf {err:.2e}")
    assert err < 1e-5
    np.testing.assert_allclose(res.trace_loss["total"], g["fit/trace/total"], rtol=1e-4)
    assert points.x_pos_numpy[-1] == sources[1][-1] == round(float(sources[1][-1])), "the integer x moved"
    _check_points("sequential fit", points, *_harness("sequential"))
    # the initial components are kept apart from the fitted ones
    np.testing.assert_array_equal(res.components_init["points"].x_pos_numpy, sources[1])


@pytest.mark.parametrize("use_log_flux", [True, False], ids=["log", "linear"])
def test_joint_fit_matches_the_harness(golden, use_log_flux):
    import jolideco_amd as jd

    _, datasets, flux_init, sources = _scene(golden)
    run32, run64 = _harness("joint", use_log_flux)
    comps = _components(flux_init, sources, use_log_flux)
    res = jd.MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV, fit_mode="joint").run(
        datasets, components=comps)
    err = rel_linf(res.components["diffuse"].flux_upsampled_numpy, run32["diffuse"])
    print(f"joint fit {'log' if use_log_flux else 'linear'}: diffuse flux rel Linf {err:.2e}")
    assert err < 1e-5
    np.testing.assert_allclose(res.trace_loss["total"], [row["total"] for row in run32["trace"]], rtol=1e-4)
    assert res.components["points"].x_pos_numpy[-1] == sources[1][-1]
    _check_points(f"joint fit {'log' if use_log_flux else 'linear'}", res.components["points"], run32, run64)


def test_sgd_fit_matches_the_harness(golden):
    import jolideco_amd as jd

    _, datasets, flux_init, sources = _scene(golden)
    run32, run64 = _harness("sequential", True, "sgd")
    res = jd.MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV, optimizer_type="sgd").run(
        datasets, components=_components(flux_init, sources))
    assert rel_linf(res.components["diffuse"].flux_upsampled_numpy, run32["diffuse"]) < 1e-5
    np.testing.assert_allclose(res.trace_loss["total"], [row["total"] for row in run32["trace"]], rtol=1e-4)
    _check_points("sgd fit", res.components["points"], run32, run64)


def test_gmm_prior_on_the_diffuse_layer_keeps_its_fused_step(golden):
    """A K = 4 synthetic 8 x 8 GMM prior on the diffuse layer (its gather kernel applies the optimizer step), an exponential
    prior on the points (backward, stepper, render) -- against the harness with the oracle's priors."""
    import jolideco_amd as jd
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    _, datasets, flux_init, sources = _scene(golden)
    n_epochs = 4
    means, covs, weights = synthetic_gmm(4, 64, seed=2)

    def oracle_priors():
        return {"diffuse": cpu_ref.GMMPatchPriorRef(cpu_ref.GMM.from_numpy(means, covs, weights, stride=4)),
                "points": cpu_ref.ExponentialPriorRef(10)}

    run32 = cases.fit_harness(datasets, flux_init, sources, n_epochs, priors=oracle_priors())
    with cpu_ref.precision(np.float64):
        run64 = cases.fit_harness(datasets, flux_init, sources, n_epochs, priors=oracle_priors())
    gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))
    comps = _components(flux_init, sources, prior_diffuse=jd.GMMPatchPrior(gmm=gmm), prior_points=jd.ExponentialPrior(alpha=10))
    deconvolver = jd.MAPDeconvolver(n_epochs=n_epochs, display_progress=False, device=DEV)
    session = deconvolver.session(datasets, components=comps)
    assert session._fuse_step(session.states[0], session.priors[0]), "the diffuse layer lost its fused step"
    assert not session._fuse_step(session.states[1], session.priors[1])
    rows = []
    for _ in range(n_epochs):
        session.epoch()
        rows.append(session.scalars.clone())
    torch.cuda.synchronize()
    err = rel_linf(session.states[0].flux_cur.cpu().numpy(), run32["diffuse"])
    print(f"gmm + exponential fit: diffuse flux rel Linf {err:.2e}")
    assert err < 1e-5
    _check_points("gmm + exponential fit", session.components["points"], run32, run64)
    n_d = session.n_d
    values = torch.stack(rows).cpu().numpy()
    totals = values[:, :n_d].sum(axis=1) - values[:, n_d : n_d + 2].sum(axis=1)
    np.testing.assert_allclose(totals, [row["total"] for row in run32["trace"]], rtol=1e-4)
    assert values[-1, n_d + 1] != 0  # (the exponential prior of the rendered image)


def test_frozen_sparse_component_stays_as_it_is(golden):
    import jolideco_amd as jd

    _, datasets, flux_init, sources = _scene(golden)
    run32 = cases.fit_harness(datasets, flux_init, sources, 3, frozen=True)
    comps = _components(flux_init, sources, frozen=True)
    image_before = comps["points"].to(DEV).flux_numpy.copy()
    res = jd.MAPDeconvolver(n_epochs=3, display_progress=False, device=DEV).run(datasets, components=comps)
    points = res.components["points"]
    np.testing.assert_array_equal(points.x_pos_numpy, sources[1])
    np.testing.assert_array_equal(points.y_pos_numpy, sources[2])
    np.testing.assert_array_equal(points._flux.detach().cpu().numpy(), cases.parameter(sources[0]))
    np.testing.assert_array_equal(points.flux_numpy, image_before)
    assert rel_linf(res.components["diffuse"].flux_upsampled_numpy, run32["diffuse"]) < 1e-5
    assert rel_linf(res.components["diffuse"].flux_upsampled_numpy, flux_init) > 1e-2  # the diffuse layer does fit
    np.testing.assert_allclose(res.trace_loss["total"], [row["total"] for row in run32["trace"]], rtol=1e-4)


@pytest.mark.parametrize("fit_mode", ["sequential", "joint"])
def test_nothing_is_captured_with_a_sparse_component(golden, monkeypatch, fit_mode):
    """JOLIDECO_GRAPH=1 asks for captured epochs; a session with a sparse component stays by value and gives its bits."""
    import jolideco_amd as jd

    _, datasets, flux_init, sources = _scene(golden)

    def fit(graph):
        monkeypatch.setenv("JOLIDECO_GRAPH", graph)
        monkeypatch.setenv("JOLIDECO_STEP_SCALARS", "device" if graph == "1" else "host")
        session = jd.MAPDeconvolver(n_epochs=8, display_progress=False, device=DEV, fit_mode=fit_mode).session(
            datasets, components=_components(flux_init, sources))
        rows = []
        for _ in range(8):
            session.epoch()
            rows.append(session.scalars.clone())
        torch.cuda.synchronize()
        points = session.components["points"]
        state = [st.flux_cur.cpu().numpy().copy() for st in session.states]
        state += [p.detach().cpu().numpy().copy() for p in (points._flux, points.x_pos, points.y_pos)]
        return state, torch.stack(rows).cpu().numpy(), len(session._graphs), session.step_scalars, session._planned_capable()

    by_value, forced = fit("0"), fit("1")
    assert forced[2] == 0 and forced[3] is None and forced[4] is False, "an epoch was planned or captured"
    for a, b in zip(forced[0], by_value[0]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(forced[1], by_value[1])

"""CPU: the sparse point-source flux component -- the oracle of tests/sparse_cases.py against the fixture
tests/golden/sparse_component.npz (generated from the live reference by tools/make_golden_sparse.py), the component's
Python surface, its FITS layout, and the refusals of what is out of scope."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sparse_cases as cases
from conftest import unpack_datasets

REPO = Path(__file__).resolve().parent.parent


def _component(use_log_flux=True, frozen=False, prior=None, shape=cases.CASE_A_SHAPE):
    import jolideco_amd as jd

    flux, x_pos, y_pos = cases.case_a()
    return jd.SparseSpatialFluxComponent.from_numpy(flux=flux, x_pos=x_pos, y_pos=y_pos, shape=shape,
                                                    use_log_flux=use_log_flux, frozen=frozen, prior=prior)


# ---------------------------------------------------------------------------------------------------- oracle, fixture
@pytest.mark.parametrize("tag,shape", [("a", cases.CASE_A_SHAPE), ("b", cases.CASE_B_SHAPE)])
@pytest.mark.parametrize("use_log_flux", [True, False], ids=["log", "linear"])
def test_oracle_matches_the_reference(golden, tag, shape, use_log_flux):
    g = golden("sparse_component")
    flux, x_pos, y_pos = (cases.case_a if tag == "a" else cases.case_b)()
    assert tuple(g[f"{tag}/shape"]) == shape
    for name, value in (("flux", flux), ("x_pos", x_pos), ("y_pos", y_pos)):
        np.testing.assert_array_equal(g[f"{tag}/{name}"], value)
    key = f"{tag}/{'log' if use_log_flux else 'linear'}"
    param = cases.parameter(flux, use_log_flux)
    image, grads = cases.oracle(param, x_pos, y_pos, shape, use_log_flux, cases.upstream(shape), dtype=np.float32)
    # (a reduction order that differs between torch builds moves the image by an ulp at most)
    np.testing.assert_allclose(image, g[f"{key}/image"], rtol=2.0**-23, atol=0)
    assert np.array_equal(image == 0, g[f"{key}/image"] == 0)
    for name, grad in zip(("grad_param", "grad_x", "grad_y"), grads):
        np.testing.assert_allclose(grad, g[f"{key}/{name}"], rtol=1e-6, atol=1e-6 * np.abs(g[f"{key}/{name}"]).max())
    image64, grads64 = cases.oracle(param, x_pos, y_pos, shape, use_log_flux, cases.upstream(shape), dtype=np.float64)
    assert cases.rel_linf(g[f"{key}/image"], image64) < 1e-6
    for name, grad64 in zip(("grad_param", "grad_x", "grad_y"), grads64):
        assert cases.rel_linf(g[f"{key}/{name}"], grad64) < 1e-5


def test_fixture_b_holds_the_edge_cases(golden):
    g = golden("sparse_component")
    H, W = cases.CASE_B_SHAPE
    flux, x_pos, y_pos = cases.case_b()
    image = g["b/linear/image"]
    # x_pos runs along the rows, y_pos along the columns
    assert image.shape == (H, W) and np.isclose(image.sum(), flux[:5].sum() + 0.5 * flux[5])
    r, c = int(x_pos[4]), int(y_pos[4])
    assert x_pos[4] == r and y_pos[4] == c and image[r, c] == flux[4]  # integer coordinates: one pixel
    assert g["b/linear/grad_x"][4] == 0 and g["b/linear/grad_y"][4] == 0
    assert y_pos[5] == W - 0.5 and np.count_nonzero(image[:, W - 1]) == 2  # half beyond the last column: its weight 0.5 stays
    for name in ("grad_param", "grad_x", "grad_y"):  # wholly outside
        assert g[f"b/linear/{name}"][6] == 0 and g[f"b/log/{name}"][6] == 0
    # sources per pixel: two in one cell (its first pixel also holds a corner of the fourth), two that share one pixel
    rows, cols = np.arange(H, dtype=np.float32)[:, None, None], np.arange(W, dtype=np.float32)[None, :, None]
    count = ((np.abs(rows - x_pos) < 1) & (np.abs(cols - y_pos) < 1)).sum(axis=-1)
    r0, c0 = int(x_pos[0]), int(y_pos[0])
    assert count[r0, c0] == 3 and count[r0 + 1, c0 + 1] == 2 and count[r0 - 1, c0 - 1] == 2
    assert np.array_equal(count > 0, image != 0)


def test_fit_harness_reproduces_the_fixture(golden):
    g = golden("sparse_component")
    datasets = unpack_datasets(g, prefix="fit/data/")
    sources = tuple(g[f"fit/start/{k}"] for k in ("flux", "x_pos", "y_pos"))
    run = cases.fit_harness(datasets, g["fit/flux_init"], sources, cases.FIT_EPOCHS, record_first_grads=True)
    assert cases.rel_linf(run["diffuse"], g["fit/diffuse"]) < 1e-6
    for key in ("flux", "x_pos", "y_pos"):
        assert cases.rel_linf(run[key], g[f"fit/{key}"]) < 1e-6, key
    np.testing.assert_allclose([row["total"] for row in run["trace"]], g["fit/trace/total"], rtol=1e-6)
    # the integer x never moves; no other first position gradient is rounding noise (Adam's first step is lr sign(g))
    assert run["x_pos"][-1] == sources[1][-1] == round(float(sources[1][-1]))
    g_x, g_y = run["first_grads"][1], run["first_grads"][2]
    largest = max(np.abs(g_x).max(), np.abs(g_y).max())
    assert g_x[-1] == 0 and all(v == 0 or abs(v) >= 1e-3 * largest for v in np.concatenate([g_x, g_y]))
    assert np.hypot(run["x_pos"] - sources[1], run["y_pos"] - sources[2]).max() > 0.5  # positions do move


# ---------------------------------------------------------------------------------------------------- Python surface
@pytest.mark.parametrize("use_log_flux", [True, False], ids=["log", "linear"])
def test_constructor_members_and_to_dict(use_log_flux):
    import jolideco_amd as jd
    from jolideco_amd.models import SparseSpatialFluxComponent

    assert jd.SparseSpatialFluxComponent is SparseSpatialFluxComponent
    flux, x_pos, y_pos = cases.case_a()
    comp = _component(use_log_flux)
    assert comp.is_sparse is True and comp.upsampling_factor == 1 and comp.use_log_flux is use_log_flux
    assert comp.shape == (1, 1) + cases.CASE_A_SHAPE and comp.wcs is None and not comp.frozen
    assert isinstance(comp.prior, jd.UniformPrior)
    np.testing.assert_array_equal(comp._flux.detach().numpy(), cases.parameter(flux, use_log_flux))
    np.testing.assert_array_equal(comp.x_pos_numpy, x_pos)
    np.testing.assert_array_equal(comp.y_pos_numpy, y_pos)
    params = list(comp.parameters())
    assert len(params) == 3 and all(p.shape == (3,) and p.dtype == torch.float32 for p in params)
    data = comp.to_dict()
    assert set(data) == {"use_log_flux", "frozen", "shape", "flux", "x_pos", "y_pos", "prior"}
    assert data["shape"] == comp.shape and data["prior"] == {"type": "uniform"} and data["frozen"] is False
    np.testing.assert_allclose(data["flux"], flux, rtol=1e-6)  # linear, whatever the parameter holds
    # the tensor constructor of the reference
    same = jd.SparseSpatialFluxComponent(flux=torch.tensor(flux), x_pos=torch.tensor(x_pos), y_pos=torch.tensor(y_pos),
                                         shape=cases.CASE_A_SHAPE, use_log_flux=use_log_flux)
    assert torch.equal(same._flux, comp._flux) and torch.equal(same.x_pos, comp.x_pos)
    with pytest.raises(ValueError, match="same length"):
        jd.SparseSpatialFluxComponent.from_numpy(flux=[1.0, 2.0], x_pos=[1.0], y_pos=[1.0], shape=(4, 4))


def test_frozen_component_has_no_parameters():
    comp = _component(frozen=True)
    assert comp.parameters() == [] and comp.to_dict()["frozen"] is True
    scalar = type(comp).from_numpy(flux=2.0, x_pos=1.0, y_pos=3.5, shape=(8, 8))
    assert scalar._flux.shape == (1,)


def test_the_image_needs_the_device():
    """There is no CPU rendering path: a component that was not moved to the HIP device says so."""
    with pytest.raises(RuntimeError, match="HIP device"):
        _component().flux


def test_flux_components_with_a_sparse_member():
    import jolideco_amd as jd

    comps = jd.FluxComponents()
    comps["diffuse"] = jd.SpatialFluxComponent.from_numpy(flux=np.ones(cases.CASE_A_SHAPE))
    comps["points"] = _component(prior=jd.ExponentialPrior(alpha=3.0))
    assert list(comps.priors) == ["diffuse", "points"] and isinstance(comps.priors["points"], jd.ExponentialPrior)
    assert len(comps.parameters()) == 4
    data = comps.to_dict()
    assert data["points"]["prior"]["type"] == "exponential" and "flux" in data["points"] and "upsampling_factor" in data["diffuse"]
    comps["points"].frozen = True
    assert len(comps.parameters()) == 1


# ---------------------------------------------------------------------------------------------------- FITS
@pytest.mark.parametrize("use_log_flux", [True, False], ids=["log", "linear"])
def test_fits_round_trip_of_a_component_file(tmp_path, use_log_flux):
    import jolideco_amd as jd
    from jolideco_amd.utils.io import IO_FORMATS_SPARSE_FLUX_COMPONENT_READ, IO_FORMATS_SPARSE_FLUX_COMPONENT_WRITE
    from jolideco_amd.utils.io._fitsfile import read_fits

    assert list(IO_FORMATS_SPARSE_FLUX_COMPONENT_READ) == ["fits"] == list(IO_FORMATS_SPARSE_FLUX_COMPONENT_WRITE)
    comp = _component(use_log_flux, frozen=True, prior=jd.InverseGammaPrior(alpha=5.0, beta=2.0), shape=(25, 31))
    filename = tmp_path / "points.fits"
    comp.write(filename)
    with pytest.raises(OSError):
        comp.write(filename)
    hdus = read_fits(filename)
    table = [hdu for hdu in hdus if hdu.kind == "bintable"][0]
    assert table.data.colnames == ["x_pos", "y_pos", "flux"]
    assert table.header["IMSHAPE1"] == 25 and table.header["IMSHAPE2"] == 31
    assert bool(table.header["LOG_FLUX"]) is use_log_flux and bool(table.header["FROZEN"]) is True
    assert table.header["PTYPE"] == "inverse-gamma"
    np.testing.assert_allclose(table.data["flux"], cases.case_a()[0], rtol=1e-6)  # the column holds the linear flux
    back = jd.SparseSpatialFluxComponent.read(filename)
    assert back.shape == (1, 1, 25, 31) and back.use_log_flux is use_log_flux and back.frozen is True
    assert isinstance(back.prior, jd.InverseGammaPrior)
    np.testing.assert_array_equal(back.x_pos_numpy, comp.x_pos_numpy)
    np.testing.assert_array_equal(back.y_pos_numpy, comp.y_pos_numpy)
    np.testing.assert_allclose(back.to_dict()["flux"], comp.to_dict()["flux"], rtol=1e-6)
    # the dense reader dispatches on the HDU type, like the reference's
    from jolideco_amd.utils.io.fits import read_flux_component_from_fits

    assert read_flux_component_from_fits(filename, hdu_name=1).is_sparse


def test_fits_round_trip_of_a_components_file(tmp_path):
    import jolideco_amd as jd
    from jolideco_amd.utils.io._fitsfile import read_fits

    comps = jd.FluxComponents()
    diffuse = np.random.RandomState(3).gamma(2.0, size=cases.CASE_A_SHAPE).astype(np.float32)
    comps["diffuse"] = jd.SpatialFluxComponent.from_numpy(flux=diffuse)
    comps["points"] = _component(use_log_flux=False)
    filename = tmp_path / "components.fits"
    comps.write(filename)
    kinds = {hdu.name: hdu.kind for hdu in read_fits(filename)}
    assert kinds["DIFFUSE"] == "image" and kinds["POINTS"] == "bintable"
    back = jd.FluxComponents.read(filename)
    assert list(back) == ["diffuse", "points"]
    assert not back["diffuse"].is_sparse and back["points"].is_sparse and back["points"].use_log_flux is False
    np.testing.assert_allclose(back["diffuse"].flux_upsampled_numpy, diffuse, rtol=1e-6)
    np.testing.assert_array_equal(back["points"].to_dict()["flux"], comps["points"].to_dict()["flux"])
    np.testing.assert_array_equal(back["points"].x_pos_numpy, comps["points"].x_pos_numpy)


def test_fits_result_carries_the_sparse_component(tmp_path):
    import jolideco_amd as jd
    from jolideco_amd.core import MAPDeconvolverResult
    from jolideco_amd.utils.table import TraceTable

    def components(x_shift):
        flux, x_pos, y_pos = cases.case_a()
        return jd.FluxComponents({
            "diffuse": jd.SpatialFluxComponent.from_numpy(flux=np.full(cases.CASE_A_SHAPE, 2.0)),
            "points": jd.SparseSpatialFluxComponent.from_numpy(flux=flux, x_pos=x_pos + x_shift, y_pos=y_pos,
                                                               shape=cases.CASE_A_SHAPE),
        })

    trace = TraceTable(names=["total", "filename"])
    trace.add_row({"total": 1.5, "filename": ""})
    result = MAPDeconvolverResult(config={"n_epochs": 1}, components=components(0.25), components_init=components(0.0),
                                  trace_loss=trace)
    filename = tmp_path / "result.fits"
    result.write(filename)
    back = MAPDeconvolverResult.read(filename)
    assert list(back.components) == ["diffuse", "points"] == list(back.components_init)
    np.testing.assert_array_equal(back.components["points"].x_pos_numpy, result.components["points"].x_pos_numpy)
    np.testing.assert_array_equal(back.components_init["points"].x_pos_numpy, cases.case_a()[1])
    assert back.components["points"].is_sparse and not back.components["diffuse"].is_sparse


@pytest.mark.parametrize("suffix,what", [(".asdf", "ASDF"), (".yaml", "YAML")])
def test_formats_without_tables_refuse_the_sparse_component(tmp_path, suffix, what):
    import jolideco_amd as jd
    from jolideco_amd.core import MAPDeconvolverResult
    from jolideco_amd.utils.table import TraceTable

    comps = jd.FluxComponents({"diffuse": jd.SpatialFluxComponent.from_numpy(flux=np.ones((8, 8))),
                               "points": _component(shape=(8, 8))})
    with pytest.raises(NotImplementedError, match="sparse flux component 'points'"):
        comps.write(tmp_path / f"components{suffix}")
    result = MAPDeconvolverResult(config={}, components=comps, trace_loss=TraceTable(names=["total", "filename"]))
    for name in ("result.asdf", "result.npz"):
        with pytest.raises(NotImplementedError, match="sparse flux component 'points'"):
            result.write(tmp_path / name)
    with pytest.raises(ValueError, match="Not a valid format"):
        comps["points"].write(tmp_path / f"points{suffix}")


# ---------------------------------------------------------------------------------------------------- the fit's edges
def _fit_inputs():
    import jolideco_amd as jd

    datasets = {"o0": {key: np.ones((8, 8), dtype=np.float32) for key in ("counts", "exposure", "background")}}
    datasets["o0"]["psf"] = np.ones((3, 3), dtype=np.float32) / 9
    comps = jd.FluxComponents({"diffuse": jd.SpatialFluxComponent.from_numpy(flux=np.ones((8, 8))),
                               "points": _component(shape=(8, 8))})
    return datasets, comps


def test_a_bare_sparse_component_is_a_type_error():
    import jolideco_amd as jd

    datasets, comps = _fit_inputs()
    deconvolver = jd.MAPDeconvolver(n_epochs=1, display_progress=False, device="cuda:0")
    with pytest.raises(TypeError, match="FluxComponents"):
        deconvolver.run(datasets, components=comps["points"])
    with pytest.raises(TypeError, match="FluxComponents"):
        deconvolver.session(datasets, components=comps["points"])


class _Sharded:
    rank, world_size, sharded, dry_run = 0, 2, True, True


def _session(deconvolver, dist=None):
    """`FitSession.__init__` up to its refusals (they come before anything touches a device)."""
    from jolideco_amd.core import FitSession
    from jolideco_amd.distributed import DistContext

    datasets, comps = _fit_inputs()
    return FitSession(deconvolver, datasets, None, comps, dist or DistContext.current())


def test_out_of_scope_combinations_are_refused(tmp_path):
    import jolideco_amd as jd

    with pytest.raises(NotImplementedError, match="sharded fit .* sparse flux component 'points'"):
        _session(jd.MAPDeconvolver(n_epochs=1, device="cuda:0", fit_mode="joint"), dist=_Sharded())
    with pytest.raises(NotImplementedError, match="compute_error=True .* sparse flux component 'points'"):
        _session(jd.MAPDeconvolver(n_epochs=1, device="cuda:0", compute_error=True))
    with pytest.raises(NotImplementedError, match="checkpoints .* sparse flux component 'points'"):
        _session(jd.MAPDeconvolver(n_epochs=1, device="cuda:0", checkpoint_path=tmp_path / "checkpoints"))


def test_sessions_with_a_sparse_component_are_never_planned():
    """`_planned_capable` is what sends an epoch to the device-resident step scalars and to graph capture."""
    from jolideco_amd.core import FitSession

    session = FitSession.__new__(FitSession)
    session.has_sparse = True
    assert session._planned_capable() is False


# ---------------------------------------------------------------------------------------------------- C ABI
def test_header_declares_the_sparse_calls():
    from jolideco_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "jolideco_hip.h").read_text(), flags=re.S)
    for name in ("jd_sparse_max_sources", "jd_sparse_render", "jd_sparse_backward"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _hip.EXPORTS
    assert "JD_KERNEL_SPARSE_RENDER = 21" in text and "JD_KERNEL_SPARSE_BACKWARD = 22" in text
    assert _hip.KERNEL_IDS["sparse_render"] == 21 and _hip.KERNEL_IDS["sparse_backward"] == 22


def test_sparse_calls_validate_their_arguments():
    """Bad arguments return JD_ERR_INVALID with a message before anything reaches a device."""
    import ctypes

    import __graft_entry__
    from jolideco_amd import _hip

    if not _hip.library_path().exists():
        __graft_entry__.build()
    lib = _hip.lib()
    limit = lib.jd_sparse_max_sources()
    assert limit >= 10_000
    assert lib.jd_kernel_name(21) == b"sparse_render_kernel" and lib.jd_kernel_name(22) == b"sparse_backward_kernel"
    p = ctypes.c_void_p(256)  # (never dereferenced: every call below returns from its argument checks)
    assert lib.jd_sparse_render(None, p, p, 3, 1, 8, 8, p, None) == -1 and b"null argument" in lib.jd_last_error()
    assert lib.jd_sparse_render(p, p, p, 3, 1, 8, 8, None, None) == -1
    assert lib.jd_sparse_render(p, p, p, 0, 1, 8, 8, p, None) == -1 and b"sources" in lib.jd_last_error()
    assert lib.jd_sparse_render(p, p, p, limit + 1, 1, 8, 8, p, None) == -1
    assert lib.jd_sparse_render(p, p, p, 3, 1, 0, 8, p, None) == -1 and b"non-positive shape" in lib.jd_last_error()
    assert lib.jd_sparse_backward(p, p, p, 3, 1, 8, 8, None, p, p, p, None) == -1
    assert lib.jd_sparse_backward(p, p, p, 3, 1, 8, -1, p, p, p, p, None) == -1
    assert lib.jd_sparse_backward(p, p, p, limit + 1, 0, 8, 8, p, p, p, p, None) == -1

"""CPU: `MultiScalePrior` -- the restatement of tests/multiscale_cases.py against the fixture tests/golden/multiscale.npz
(written from the live reference by tools/make_golden_multiscale.py), the host logic of the prior (constructor, weights,
draw order, `to_dict`, refusals) and the C-ABI of the two pyramid kernels (declared, bound, validating their arguments)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import multiscale_cases as cases
from conftest import rel_linf, unpack_datasets
from jolideco_amd import MultiScalePrior  # noqa: F401  (every test of this file is about it)

REPO = Path(__file__).resolve().parent.parent


def _inner(case=None, **kwargs):
    from jolideco_amd import GMMPatchPrior
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    case = case or cases.CASES["32x40-L2"]
    gmm = GaussianMixtureModel.from_numpy(*cases.case_mixture(case), meta=GaussianMixtureModelMeta(stride=case["stride"]))
    return GMMPatchPrior(gmm=gmm, **kwargs)


# ------------------------------------------------------------------------------------------- the restatement and the fixture
@pytest.mark.parametrize("name", list(cases.CASES))
def test_restatement_reproduces_the_fixture(golden, name):
    """Where the reference can run (outer cycle spin off) the float32 restatement with the reference's FFT blur gives the
    reference's bits; the direct-sum form the GPU tests use lies as close to the float64 restatement as the reference
    does, up to a factor.  The outer cycle-spin cases hold the restatement's own numbers."""
    g, case = golden("multiscale"), cases.CASES[name]
    assert np.array_equal(g[f"{name}/flux"], cases.case_flux(case))
    assert cases.mixture_checksum(cases.case_mixture(case)) == pytest.approx(float(g[f"{name}/gmm_checksum"]), rel=1e-13)
    stored = [None if tuple(s) == (-99, -99) else tuple(int(v) for v in s) for s in g[f"{name}/draws"]]
    assert tuple(stored) == cases.draws(case)
    o32, o64 = cases.cached_restate(name, "float32"), cases.cached_restate(name, "float64")
    value, grad = float(g[f"{name}/value"]), g[f"{name}/grad"]
    if bool(g[f"{name}/from_reference"]):
        assert name in cases.REFERENCE_CASES
        fft32 = cases.restate(case, np.float32, conv=cases.conv_same_fft)
        assert fft32["value"] == value and np.array_equal(fft32["grad"].astype(np.float32), grad)
        ref_v, ref_g = abs(value - o64["value"]) / abs(o64["value"]), rel_linf(grad, o64["grad"])
        err_v, err_g = abs(o32["value"] - o64["value"]) / abs(o64["value"]), rel_linf(o32["grad"], o64["grad"])
        print(f"multiscale {name}: against float64, value reference {ref_v:.1e} direct {err_v:.1e} | gradient reference {ref_g:.1e} "
              f"direct {err_g:.1e}")
        assert err_v <= max(4 * ref_v, 1e-6) and err_g <= max(4 * ref_g, 1e-6)
    else:
        assert case["outer_spin"]
        assert o32["value"] == pytest.approx(value, rel=1e-6) and rel_linf(o32["grad"], grad) < 1e-6
    if not case["marginalize"]:
        assert cases.margins(o64["levels"]).min() == pytest.approx(float(g[f"{name}/min_margin"]), rel=1e-6)


def test_restatement_structure():
    """The pieces: ragged pooling floors, a zero weight skips the level AND its blur, the blur is cumulative."""
    case = cases.CASES["33x41-L3"]
    levels = cases.cached_restate("33x41-L3", "float64")["levels"]
    assert [d["pooled"].shape for d in levels] == [(33, 41), (16, 20), (8, 10)]
    skipped = cases.cached_restate("skip-level", "float64")["levels"]
    assert [d["level"] for d in skipped] == [0, 2]
    flux = torch.from_numpy(cases.case_flux(cases.CASES["skip-level"]).astype(np.float64))[None, None]
    g = cases.conv_same_direct(flux, torch.from_numpy(cases.level_kernel(0).astype(np.float64)))
    g = cases.conv_same_direct(g, torch.from_numpy(cases.level_kernel(2).astype(np.float64)))  # (not level 1's kernel)
    expected = torch.nn.functional.avg_pool2d(g, 4).numpy()[0, 0]
    np.testing.assert_allclose(skipped[1]["pooled"], expected, rtol=1e-12)
    assert [cases.level_kernel(level).shape[0] for level in range(5)] == [3, 7, 11, 23, 43]
    assert case["shape"] == (33, 41)


def test_numpy_kernel_formulas_agree_with_torch():
    """`down_numpy` / `up_numpy` (the oracle of the kernel tests) against torch's conv2d / avg_pool2d and autograd."""
    rs = np.random.RandomState(5)
    for shape, f, n_taps in cases.KERNEL_CASES:
        taps = cases.kernel_taps(n_taps, 7)
        x = rs.gamma(20, size=shape)
        g, d = cases.down_numpy(x, f, taps, shifts=(3, -2))
        t = torch.from_numpy(np.roll(x, (3, -2), axis=(0, 1)))[None, None].requires_grad_(True)
        kernel = torch.from_numpy(np.outer(taps.astype(np.float64), taps.astype(np.float64)))
        gt = cases.conv_same_direct(t, kernel)
        dt = torch.nn.functional.avg_pool2d(gt, f)
        np.testing.assert_allclose(g, gt.detach().numpy()[0, 0], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(d, dt.detach().numpy()[0, 0], rtol=1e-12, atol=1e-12)
        dd, dg = rs.normal(size=d.shape), rs.normal(size=shape)
        (torch.sum(dt * torch.from_numpy(dd)) + torch.sum(gt * torch.from_numpy(dg))).backward()
        np.testing.assert_allclose(cases.up_numpy(dd, dg, shape, f, taps), t.grad.numpy()[0, 0], rtol=1e-11, atol=1e-12)


def test_fit_restatement_reproduces_the_fixture(golden):
    """The 6-epoch fit: `cpu_ref.map_fit_sequential` over the restatement (FFT blur) gives the bits of the reference's run."""
    from oracle import cpu_ref

    g = golden("multiscale")
    datasets, flux_init, arrays = cases.fit_inputs()
    stored = unpack_datasets(g, prefix="fit/data/")
    assert all(np.array_equal(stored[n][k], datasets[n][k]) for n in datasets for k in datasets[n])
    assert np.array_equal(g["fit/flux_init"], flux_init)
    fit = cases.FIT
    gmm = cpu_ref.GMM.from_numpy(*arrays, stride=fit["stride"])
    prior = cases.MultiScalePriorRef(gmm, fit["stride"], fit["n_levels"], conv=cases.conv_same_fft)
    final, trace = cpu_ref.map_fit_sequential(datasets, {"flux": flux_init}, {"flux": prior}, n_epochs=fit["n_epochs"])
    assert np.array_equal(final["flux"], g["fit/flux_final"])
    assert trace[-1]["total"] == g["fit/trace/total"][-1]


# ------------------------------------------------------------------------------------------------------------- host logic
def test_exports_and_registry():
    import jolideco_amd as jd
    from jolideco_amd import priors

    assert jd.MultiScalePrior is priors.MultiScalePrior and "MultiScalePrior" in jd.__all__ and "MultiScalePrior" in priors.__all__
    assert priors.MultiScalePrior not in priors.PRIOR_REGISTRY.values()  # (the reference does not register it either)


def test_constructor_weights_and_flags():
    from jolideco_amd import MultiScalePrior, SmoothnessPrior, UniformPrior

    prior = MultiScalePrior(_inner())
    assert (prior.n_levels, prior.cycle_spin, prior.anti_alias) == (2, True, True)
    assert np.array_equal(prior.weights.numpy(), cases.level_weights(2).numpy())
    assert prior.shift_kind == "levels"
    assert (prior.shardable, prior.supports_fused_step, prior.supports_phases) == (False, False, False)
    assert tuple(prior.patch_shape) == (8, 8)
    assert not list(prior.parameters()) or all(p is not prior._log_weights for p in prior.parameters())  # constants
    skip = MultiScalePrior(_inner(), n_levels=3, weights=[0.6, 0.0, 0.4])
    assert np.array_equal(skip.weights.numpy(), cases.level_weights(3, [0.6, 0.0, 0.4]).numpy()) and float(skip.weights[1]) == 0.0
    assert [(level, f) for level, f, _ in skip.levels] == [(0, 1), (2, 4)]
    assert skip.levels[1][2] == float(16 * cases.level_weights(3, [0.6, 0.0, 0.4])[2])
    with pytest.raises(ValueError, match="n_levels"):
        MultiScalePrior(_inner(), n_levels=6)
    with pytest.raises(ValueError, match="weights"):
        MultiScalePrior(_inner(), n_levels=2, weights=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="MultiScalePrior"):
        MultiScalePrior(MultiScalePrior(_inner()))
    with pytest.raises(ValueError, match="inner prior"):
        MultiScalePrior(object())
    with pytest.raises(ValueError, match="patch shape / generator"):
        MultiScalePrior(SmoothnessPrior(width=1))  # (the outer cycle spin draws from the inner prior's generator)
    assert MultiScalePrior(SmoothnessPrior(width=1), cycle_spin=False).draw_shifts() == (None, None, None)
    assert MultiScalePrior(UniformPrior(), cycle_spin=False).n_levels == 2


def test_level_taps_reproduce_the_reference_kernels():
    from jolideco_amd.priors.patches.core import multiscale_level_taps

    for level, n_taps in enumerate([3, 7, 11, 23, 43]):
        taps = np.array(multiscale_level_taps(level))
        assert taps.size == n_taps and np.array_equal(taps, taps[::-1])
        kernel = cases.level_kernel(level).astype(np.float64)
        assert np.abs(np.outer(taps, taps) - kernel).max() <= 2.0**-22 * kernel.max()  # (two float32 roundings)
    assert multiscale_level_taps(3, anti_alias=False) == [1.0]


@pytest.mark.parametrize("name", ["inner-spin", "outer-spin", "outer-inner-spin", "skip-level"])
def test_draw_order_matches_the_fixture(golden, name):
    """One draw: the outer roll first, then one entry per level, ascending; None for a skipped level or a prior that does
    not spin -- the fixture's draws are the reference's (inner) and the restatement's (outer)."""
    from jolideco_amd import MultiScalePrior

    case = cases.CASES[name]
    generator = torch.Generator(device="cpu")
    if case["inner_seed"] is not None:
        generator.manual_seed(case["inner_seed"])
    prior = MultiScalePrior(_inner(case, cycle_spin=case["inner_spin"], generator=generator), n_levels=case["n_levels"],
                            weights=case["weights"], cycle_spin=case["outer_spin"])
    stored = tuple(None if tuple(s) == (-99, -99) else tuple(int(v) for v in s) for s in golden("multiscale")[f"{name}/draws"])
    assert prior.draw_shifts() == stored and prior.last_shifts == stored
    assert len(stored) == 1 + case["n_levels"]
    again = prior.draw_shifts_many(2)
    assert len(again) == 2 and all(len(d) == 1 + case["n_levels"] for d in again)


def test_to_dict_has_the_reference_keys():
    from jolideco_amd import MultiScalePrior

    inner = _inner()
    data = MultiScalePrior(inner, n_levels=3, weights=[0.6, 0.0, 0.4], cycle_spin=False, anti_alias=False).to_dict()
    assert list(data) == ["n_levels", "weights", "cycle_spin", "anti_alias", "prior"]
    assert data["n_levels"] == 3 and data["cycle_spin"] is False and data["anti_alias"] is False
    assert data["weights"] == cases.level_weights(3, [0.6, 0.0, 0.4]).numpy().tolist()
    assert data["prior"] == inner.to_dict()


def test_refusals(tmp_path):
    import jolideco_amd as jd
    from jolideco_amd.core import FitSession, MAPDeconvolverResult
    from jolideco_amd.distributed import DistContext
    from jolideco_amd.utils.table import TraceTable

    prior = jd.MultiScalePrior(_inner(), n_levels=3, cycle_spin=False)
    with pytest.raises(NotImplementedError, match="MultiScalePrior"):
        prior.check_hessian_ones()
    with pytest.raises(NotImplementedError, match="MultiScalePrior"):
        prior.hessian_ones(torch.ones(1, 1, 32, 32))
    with pytest.raises(ValueError, match="level 2 of a 20 x 40 image is 5 x 10: smaller than the inner patch"):
        prior.device_fwd_bwd(torch.ones(1, 1, 20, 40), torch.zeros(1))
    comps = jd.FluxComponents({"flux": jd.SpatialFluxComponent.from_numpy(flux=np.ones((32, 32)), prior=prior)})
    for suffix in (".fits", ".yaml", ".asdf"):
        with pytest.raises(NotImplementedError, match="MultiScalePrior of the flux component 'flux'"):
            comps.write(tmp_path / f"components{suffix}")
    for suffix in (".fits", ".yaml"):
        with pytest.raises(NotImplementedError, match="MultiScalePrior"):
            comps["flux"].write(tmp_path / f"component{suffix}")
    result = MAPDeconvolverResult(config={}, components=comps, trace_loss=TraceTable(names=["total", "filename"]))
    for name in ("result.fits", "result.asdf", "result.npz"):
        with pytest.raises(NotImplementedError, match="MultiScalePrior"):
            result.write(tmp_path / name)
    assert not list(tmp_path.iterdir())
    datasets = {"o0": {key: np.ones((32, 32), dtype=np.float32) for key in ("counts", "exposure", "background")}}
    datasets["o0"]["psf"] = np.ones((3, 3), dtype=np.float32) / 9
    # (`FitSession.__init__` up to its refusals: they come before anything touches a device)
    with pytest.raises(NotImplementedError, match="checkpoints .* MultiScalePrior of the flux component 'flux'"):
        FitSession(jd.MAPDeconvolver(n_epochs=1, device="cuda:0", checkpoint_path=tmp_path / "checkpoints"), datasets, None,
                   comps, DistContext.current())
    with pytest.raises(NotImplementedError, match="compute_error=True is not implemented for a MultiScalePrior"):
        FitSession(jd.MAPDeconvolver(n_epochs=1, device="cuda:0", compute_error=True), datasets, None, comps,
                   DistContext.current())


def test_sessions_with_the_prior_are_never_planned():
    from jolideco_amd.core import FitSession

    session = FitSession.__new__(FitSession)
    session.has_sparse, session.has_multiscale = False, True
    assert session._planned_capable() is False


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_header_declares_the_multiscale_calls():
    from jolideco_amd import _hip

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "jolideco_hip.h").read_text(), flags=re.S)
    for name in ("jd_multiscale_down", "jd_multiscale_up_adjoint", "jd_multiscale_value"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _hip.EXPORTS
    assert "JD_KERNEL_MULTISCALE_DOWN = 23" in text and "JD_KERNEL_MULTISCALE_UP = 24" in text and "JD_KERNEL_COUNT = 25" in text
    assert _hip.KERNEL_IDS["multiscale_down"] == 23 and _hip.KERNEL_IDS["multiscale_up"] == 24
    assert "multiscale.hip" in (REPO / "jolideco_amd" / "csrc" / "Makefile").read_text()


def test_multiscale_calls_validate_their_arguments():
    """Bad arguments return JD_ERR_INVALID with a message before anything reaches a device."""
    import __graft_entry__
    from jolideco_amd import _hip

    if not _hip.library_path().exists():
        __graft_entry__.build()
    lib = _hip.lib()
    assert lib.jd_kernel_name(23) == b"multiscale_down_kernel" and lib.jd_kernel_name(24) == b"multiscale_up_kernel"
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(512)  # (never dereferenced: every call below returns from its argument checks)
    taps = (ctypes.c_float * 45)(*([1.0] * 45))

    def down(src=p, H=32, W=40, f=2, t=taps, n=7, sy=0, sx=0, g_out=q, d_out=p, dd=None):
        return lib.jd_multiscale_down(src, H, W, f, t, n, sy, sx, g_out, d_out, dd, None)

    def up(dg=q, dd=p, H=32, W=40, f=2, t=taps, n=7, out=p, rolled=0, sy=0, sx=0, vals=None, coefs=None, n_values=0, value=None):
        return lib.jd_multiscale_up_adjoint(dg, dd, H, W, f, t, n, out, rolled, sy, sx, vals, coefs, n_values, value, None)

    for call in (down, up):
        assert call(t=None) == -1 and b"null argument" in lib.jd_last_error()
        for f in (0, 3, 32, -2):
            assert call(f=f) == -1 and b"pooling factor" in lib.jd_last_error()
        for n in (0, 2, 8, 45, -1):
            assert call(n=n) == -1 and b"taps" in lib.jd_last_error()
        assert call(H=7, f=8) == -1 and b"smaller than the pooling factor" in lib.jd_last_error()
        assert call(W=1, f=2) == -1
        assert call(sy=32) == -1 and b"roll" in lib.jd_last_error()
        assert call(sx=-1) == -1
    assert down(src=None) == -1 and b"null argument" in lib.jd_last_error()
    assert down(d_out=None) == -1
    assert down(g_out=p) == -1 and b"alias" in lib.jd_last_error()
    assert up(dd=None) == -1 and b"null argument" in lib.jd_last_error()
    assert up(out=None) == -1
    assert up(dg=p) == -1 and b"alias" in lib.jd_last_error()
    assert up(rolled=0, sy=1) == -1 and b"accumulating form" in lib.jd_last_error()
    coefs = (ctypes.c_float * 6)(*([1.0] * 6))
    assert up(value=p, vals=None, coefs=coefs, n_values=2) == -1 and b"null argument" in lib.jd_last_error()
    assert up(value=p, vals=p, coefs=coefs, n_values=6) == -1 and b"level values" in lib.jd_last_error()
    assert lib.jd_multiscale_value(p, coefs, 2, None, None) == -1 and b"null argument" in lib.jd_last_error()
    assert lib.jd_multiscale_value(None, coefs, 2, p, None) == -1
    assert lib.jd_multiscale_value(p, coefs, 0, p, None) == -1 and b"level values" in lib.jd_last_error()

"""GPU: the GMM patch prior with a sub-pixel cycle spin (`SubpixelGMMPatchPrior`; csrc/gmm_subpix.hip): a staging kernel
writes S = the 3 x 3 stencil of the rolled, normed image in front of the unchanged pass, an adjoint kernel carries the
pass's gradient with respect to S back to the raw flux.

Oracle: tests/gmm_subpix_cases.py (torch.roll + F.conv2d + `oracle/cpu_ref`), pinned against the live reference by
tests/golden/gmm_subpix.npz.  Its float64 evaluation is the arbiter; the float32 oracle's own distance from it, e_ref,
sets the tolerance -- the project's rule of tests/test_gpu_image_norm.py: value <= max(3e-6, 4 e_ref), gradient <=
max(1e-5, 4 e_ref); max mode: the arg-max equal on every patch whose float64 margin is at least NEAR_TIE, and the pixels a
near-tie patch reaches (at most 1 % of the patches, tests/test_gmm_subpix_golden.py) left out of the gradient comparison.
Measured figures: profiles/gmm_subpix/README.md.
"""
import numpy as np
import pytest
import torch

import gmm_subpix_cases as cases
from conftest import rel_linf, unpack_datasets
from image_norm_cases import make_norm
from tools import gmm16_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(arrays, stride=4):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


@pytest.fixture(scope="module")
def model(golden):
    return _model(cases.fixture_gmm(golden))


@pytest.fixture(scope="module")
def model256():
    return _model(cases.mixture256(), stride=gmm16_cases.STRIDE)


def _std():
    from jolideco_amd.utils.norms import StandardizedSubtractMeanPatchNorm

    return StandardizedSubtractMeanPatchNorm()


def _n_patches(shape, stride, patch):
    return ((shape[0] - patch) // stride + 1) * ((shape[1] - patch) // stride + 1)


def _dev(array):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(DEV)


def _evaluate(model, flux, stride, roll, offsets, marginalize=False, grad_init=None, coef=1.0, want_argmax=False, norm=None,
              patch_norm=None, value_init=None, want_grad=True):
    """(value, gradient image, arg-max) of one low-level call with value scale 1 (the sum over the patches); `offsets`
    None: the existing pass (no sub-pixel cycle spin); `value_init`: the call accumulates its value onto that number."""
    handle = model.handle(DEV)
    value = torch.full((1,), np.nan if value_init is None else value_init, device=DEV)
    grad = None
    if want_grad:
        grad = torch.zeros_like(flux) if grad_init is None else grad_init.clone()
    patch = 8 if handle.D == 64 else 16
    argmax = torch.full((_n_patches(flux.shape, stride, patch),), -7, dtype=torch.int32, device=DEV) if want_argmax else None
    handle.prior_fwd_bwd(flux, stride, roll, value, 1.0, grad=grad, grad_coef=coef, marginalize=marginalize, argmax_out=argmax,
                         norm=norm, patch_norm=patch_norm, subpix=offsets, accumulate_value=value_init is not None)
    torch.cuda.synchronize()
    return float(value), None if grad is None else grad.cpu().numpy(), None if argmax is None else argmax.cpu().numpy()


def _check(label, o64, o32, model, flux_np, stride, roll, offsets, marginalize, patch=8, **kwargs):
    """The protocol of the module docstring on one case: value (assigned and accumulated), arg-max on clear patches, and
    the gradient accumulated with coef = 0.75 into a non-zero image"""
    shape = flux_np.shape
    total64, d64, arg64, margin = o64
    total32, d32, _, _ = o32
    keep = np.ones(shape, dtype=bool)
    clear = None
    if not marginalize:
        clear = margin >= cases.NEAR_TIE
        assert (~clear).sum() <= 0.01 * clear.size
        keep = ~cases.near_tie_mask(margin, shape, stride, roll, patch=patch)
    e_ref_value = abs(total32 - total64) / abs(total64)
    e_ref_grad = cases.rel_err(d32, d64, keep)
    g0 = np.random.RandomState(shape[1]).normal(size=shape).astype(np.float32) * np.float32(np.abs(d64).max())
    coef = 0.75
    value, grad, argmax = _evaluate(model, _dev(flux_np), stride, roll, offsets, marginalize, _dev(g0), coef,
                                    want_argmax=not marginalize, **kwargs)
    v0 = 1000.0
    value_acc, _, _ = _evaluate(model, _dev(flux_np), stride, roll, offsets, marginalize, value_init=v0, want_grad=False, **kwargs)
    e_value = abs(value - total64) / abs(total64)
    e_value_acc = abs((value_acc - v0) - total64) / abs(total64)
    expected = g0.astype(np.float64) + coef * d64
    err = np.abs(grad - expected) / np.abs(coef * d64).max()
    e_grad = float(err[keep].max())
    edge = cases.near_border_or_seam(shape, roll) & keep
    e_edge = float(err[edge].max()) if edge.any() else 0.0
    print(f"gmm subpix parity {label} {'lse' if marginalize else 'max'} {shape} stride {stride} roll {roll} offsets {offsets}: "
          f"value e_ref {e_ref_value:.2e} device {e_value:.2e} accumulated {e_value_acc:.2e} | gradient e_ref {e_ref_grad:.2e} "
          f"device {e_grad:.2e}, within one of a border or the seam {e_edge:.2e} ({int(edge.sum())} pixels)")
    assert np.abs(d64).max() > 0 and np.isfinite(grad).all() and np.isfinite(value)
    assert e_value <= max(3e-6, 4 * e_ref_value)
    assert e_value_acc <= max(3e-6, 4 * e_ref_value)
    assert e_grad <= max(1e-5, 4 * e_ref_grad)
    if not marginalize:
        assert np.array_equal(argmax[clear], arg64[clear])


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("index", range(len(cases.CASES)))
@pytest.mark.parametrize("marginalize", [False, True])
def test_prior_matches_the_oracle(golden, model, marginalize, index):
    shape, stride, roll, offsets = cases.CASES[index]
    o64 = cases.cached_oracle(golden, index, marginalize, np.float64)
    o32 = cases.cached_oracle(golden, index, marginalize, np.float32)
    _check(f"case {index}", o64, o32, model, cases.case_flux(index), stride, roll, offsets, marginalize)


# ------------------------------------------------------------------------------------------------ 2. offsets (0, 0)
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("norm_type", [None, "asinh"])
def test_zero_offsets_are_the_existing_pass_bit_for_bit(model, model256, norm_type, d):
    """Offsets (0, 0): the centre weight is 1 and the rest are 0, so nothing is rounded -- value, gradient (accumulated into a
    non-zero image) and arg-max of the existing pass on the same flux and roll"""
    norm = None if norm_type is None else make_norm(norm_type)
    mdl, stride = (model, 4) if d == 64 else (model256, 8)
    for shape, roll in (((40, 44), (2, -1)), ((37, 41), (-1, 2)), ((72, 100), None)):
        flux = _dev(np.random.RandomState(shape[0]).gamma(20, size=shape))
        g0 = _dev(np.random.RandomState(1).normal(size=shape))
        plain = _evaluate(mdl, flux, stride, roll, None, False, g0, -0.7, want_argmax=True, norm=norm)
        spun = _evaluate(mdl, flux, stride, roll, (0.0, 0.0), False, g0, -0.7, want_argmax=True, norm=norm)
        assert spun[0] == plain[0] and np.array_equal(spun[1], plain[1]) and np.array_equal(spun[2], plain[2]), (shape, roll)
        assert np.abs(plain[1] - g0.cpu().numpy()).max() > 0 and (plain[2] >= 0).all()


# ------------------------------------------------------------------------------------------------ 3. norms, patch norm, D = 256
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("norm_type", ["asinh", "log"])
def test_image_norms(golden, model, norm_type, marginalize):
    """(37, 41): the scalar paths of both kernels, n applied per staged pixel, n' on the raw flux"""
    index = 2
    shape, stride, roll, offsets = cases.CASES[index]
    o64 = cases.cached_oracle(golden, index, marginalize, np.float64, norm_type=norm_type)
    o32 = cases.cached_oracle(golden, index, marginalize, np.float32, norm_type=norm_type)
    _check(norm_type, o64, o32, model, cases.case_flux(index), stride, roll, offsets, marginalize, norm=make_norm(norm_type))


def test_standardized_patch_norm(golden, model):
    index = 0
    shape, stride, roll, offsets = cases.CASES[index]
    o64 = cases.cached_oracle(golden, index, False, np.float64, patch_norm="std-subtract-mean")
    o32 = cases.cached_oracle(golden, index, False, np.float32, patch_norm="std-subtract-mean")
    _check("std-subtract-mean", o64, o32, model, cases.case_flux(index), stride, roll, offsets, False, patch_norm=_std())


@pytest.mark.parametrize("index", range(len(cases.CASES_256)))
@pytest.mark.parametrize("marginalize", [False, True])
def test_16x16_patches(golden, model256, marginalize, index):
    shape, stride, roll, offsets = cases.CASES_256[index]
    o64 = cases.cached_oracle(golden, index, marginalize, np.float64, table=256)
    o32 = cases.cached_oracle(golden, index, marginalize, np.float32, table=256)
    _check(f"D = 256 case {index}", o64, o32, model256, cases.case_flux(index, cases.CASES_256), stride, roll, offsets, marginalize,
           patch=16)


# ------------------------------------------------------------------------------------------------ 4. device-resident scalars
@pytest.mark.parametrize("index", [0, 2, 9])
def test_device_resident_roll_and_offsets_give_the_same_bits(model, index):
    """`shift_dev` + `offset_dev`, with garbage in the by-value arguments, against the by-value call"""
    from jolideco_amd.ops import DeviceShifts

    shape, stride, roll, offsets = cases.CASES[index]
    flux = _dev(cases.case_flux(index))
    g0 = _dev(np.random.RandomState(3).normal(size=shape))
    by_value = _evaluate(model, flux, stride, roll, offsets, False, g0, 0.5, want_argmax=True)
    roll_dev = DeviceShifts(torch.tensor([roll[0] % shape[0], roll[1] % shape[1]], dtype=torch.int32, device=DEV), (17, -23))
    offsets_dev = DeviceShifts(torch.tensor(offsets, dtype=torch.float32, device=DEV), (0.49, -0.01))
    on_device = _evaluate(model, flux, stride, roll_dev, offsets_dev, False, g0, 0.5, want_argmax=True)
    assert on_device[0] == by_value[0] and np.array_equal(on_device[1], by_value[1]) and np.array_equal(on_device[2], by_value[2])
    assert np.abs(by_value[1] - g0.cpu().numpy()).max() > 0


# ------------------------------------------------------------------------------------------------ 5. repeatability
def test_two_runs_give_the_same_bits(model):
    shape, stride, roll, offsets = cases.CASES[8]
    flux = _dev(cases.case_flux(8))
    runs = [_evaluate(model, flux, stride, roll, offsets, False, None, 1.0, want_argmax=True) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert np.abs(runs[0][1]).max() > 0


# ------------------------------------------------------------------------------------------------ 6. forward only
@pytest.mark.parametrize("d", [64, 256])
def test_forward_only_gives_the_same_value_and_touches_no_gradient(model, model256, d):
    mdl = model if d == 64 else model256
    shape, stride, roll, offsets = cases.CASES[0] if d == 64 else cases.CASES_256[0]
    flux = _dev(cases.case_flux(0, None if d == 64 else cases.CASES_256))
    g0 = _dev(np.random.RandomState(4).normal(size=shape))
    both = _evaluate(mdl, flux, stride, roll, offsets, False, g0, 0.5)
    # (the gradient image of the call before stays in the handle; a forward-only call must neither read nor change ours)
    grad = g0.clone()
    handle = mdl.handle(DEV)
    value = torch.zeros(1, device=DEV)
    handle.prior_fwd_bwd(flux, stride, roll, value, 1.0, grad=None, subpix=offsets)
    torch.cuda.synchronize()
    assert float(value) == both[0]
    assert np.array_equal(grad.cpu().numpy(), g0.cpu().numpy())
    again = _evaluate(mdl, flux, stride, roll, offsets, False, g0, 0.5)
    assert again[0] == both[0] and np.array_equal(again[1], both[1])


# ------------------------------------------------------------------------------------------------ 7. autograd
def test_autograd_equals_the_fused_path(model):
    """`prior(flux).backward()`: same value and gradient as `device_fwd_bwd` with the same draw"""
    from jolideco_amd import SubpixelGMMPatchPrior

    prior = SubpixelGMMPatchPrior(gmm=model, norm=make_norm("asinh"), generator=torch.Generator("cpu").manual_seed(21))
    flux = _dev(np.random.RandomState(37).gamma(20, size=(37, 41))).reshape(1, 1, 37, 41).requires_grad_(True)
    value = prior(flux)
    value.backward()
    drawn = prior.last_shifts
    assert drawn == cases.draw(torch.Generator("cpu").manual_seed(21))
    ref_v, ref_g = torch.zeros(1, device=DEV), torch.zeros((37, 41), device=DEV)
    prior.device_fwd_bwd(flux.detach(), ref_v, grad=ref_g, coef=1.0, shifts=drawn)
    torch.cuda.synchronize()
    assert float(value.detach()) == float(ref_v)
    assert np.array_equal(flux.grad.cpu().numpy()[0, 0], ref_g.cpu().numpy()) and np.abs(ref_g.cpu().numpy()).max() > 0


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_are_error_returns_and_leave_the_handle_usable(golden, model):
    from jolideco_amd import SubpixelGMMPatchPrior

    shape, stride, roll, offsets = cases.CASES[0]
    flux = _dev(cases.case_flux(0))
    before = _evaluate(model, flux, stride, roll, offsets)
    with pytest.raises(RuntimeError, match=r"offsets .* not in \[-0.5, 0.5\]"):
        _evaluate(model, flux, stride, roll, (0.6, 0.0))
    with pytest.raises(RuntimeError, match=r"offsets .* not in \[-0.5, 0.5\]"):
        _evaluate(model, flux, stride, roll, (0.0, float("nan")))
    with pytest.raises(RuntimeError, match="smaller than a patch"):
        _evaluate(model, _dev(np.ones((7, 40))), stride, roll, offsets)
    prior = SubpixelGMMPatchPrior(gmm=model)
    with pytest.raises(NotImplementedError, match="fused optimizer step"):
        prior.device_fwd_bwd_step(flux, torch.zeros(1, device=DEV), 1.0, None)
    with pytest.raises(ValueError, match="whole prior"):
        model.handle(DEV).prior_fwd_bwd(flux, stride, roll, torch.zeros(1, device=DEV), 1.0, subpix=offsets, patch_rows=(0, 2))
    after = _evaluate(model, flux, stride, roll, offsets)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    total64 = cases.cached_oracle(golden, 0, False, np.float64)[0]
    assert abs(after[0] - total64) <= 3e-6 * abs(total64)


# ------------------------------------------------------------------------------------------------ 9. fits
def _fit_components(golden):
    from jolideco_amd import SpatialFluxComponent, SubpixelGMMPatchPrior
    from image_norm_cases import fixture_gmm

    g = golden("gmm_subpix")
    prior = SubpixelGMMPatchPrior(gmm=_model(fixture_gmm(golden, "fit/gmm/")))
    return g, unpack_datasets(g, "fit/data/"), SpatialFluxComponent.from_numpy(flux=g["fit/flux_init"], prior=prior)


def test_sequential_fit_matches_the_reference(golden):
    """6 sequential epochs of a 32 x 32 scene, two observations, default generators, through `MAPDeconvolver.run()`"""
    from jolideco_amd import MAPDeconvolver

    g, datasets, comp = _fit_components(golden)
    res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).run(datasets, components=comp)
    err = rel_linf(res.flux_total, g["fit/flux_final"])
    print(f"gmm subpix fit: flux rel Linf {err:.2e}")
    assert err < 1e-5
    np.testing.assert_allclose(res.trace_loss["total"], g["fit/trace/total"], rtol=1e-4)


def test_joint_fit_runs_by_value_and_equals_its_replay(golden, monkeypatch):
    """A 2-dataset joint fit with the component: the session reports by-value epochs, captures nothing, and the same fit with
    the step scalars forced to the host (the by-value form throughout) gives the same bits"""
    from jolideco_amd import MAPDeconvolver

    out = []
    for mode in ("auto", "host"):
        if mode == "host":
            monkeypatch.setenv("JOLIDECO_STEP_SCALARS", "host")
        _, datasets, comp = _fit_components(golden)
        session = MAPDeconvolver(n_epochs=5, display_progress=False, device=DEV, fit_mode="joint").session(datasets, components=comp)
        assert session.has_subpix_patches and not session._planned_capable()
        assert not session._fuse_step(session.states[0], session.priors[0])
        rows = []
        for _ in range(5):
            session.epoch()
            rows.append(session.scalars.clone())
        torch.cuda.synchronize()
        assert session.graph_policy.startswith("by value") and not session._graphs
        out.append((session.states[0].flux_cur.cpu().numpy().copy(), torch.stack(rows).cpu().numpy(), session.priors[0].last_shifts))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert np.isfinite(out[0][0]).all() and not np.array_equal(out[0][0], golden("gmm_subpix")["fit/flux_init"].astype(np.float32))

"""GPU: the GMM patch prior with a jittered patch grid (`JitteredGMMPatchPrior`; csrc/gmm_jitter.hip): a staging kernel lays
the jittered patches of the rolled, normed image side by side in front of the unchanged pass, an adjoint kernel gathers the
pass's gradient back to the raw flux.

Oracle: tests/gmm_jitter_cases.py (torch.roll + fancy indexing + `oracle/cpu_ref`), pinned against the live reference by
tests/golden/gmm_jitter.npz.  Its float64 evaluation is the arbiter; the float32 oracle's own distance from it, e_ref, sets the
tolerance: value (assigned and accumulated) <= max(3e-6, 4 e_ref), gradient (accumulated with coefficient 0.75 into a non-zero
image) <= max(1e-5, 4 e_ref); max mode: the arg-max equal on every patch whose float64 margin is at least NEAR_TIE, and the
pixels a near-tie patch covers (at most 1 % of the patches, tests/test_gmm_jitter_golden.py; no case has one) left out of
the gradient comparison.  Measured figures: profiles/gmm_jitter/README.md.
"""
import numpy as np
import pytest
import torch

import gmm_jitter_cases as cases
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


def _dev(array):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(DEV)


def _evaluate(model, flux, stride, roll, jitter, marginalize=False, grad_init=None, coef=1.0, want_argmax=False, norm=None,
              patch_norm=None, value_init=None, want_grad=True):
    """(value, gradient image, arg-max) of one low-level call with value scale 1 (the sum over the patches); `jitter` =
    (jitter_y, jitter_x), host arrays or device tensors; None: the existing pass; `value_init`: the call accumulates its value
    onto that number."""
    handle = model.handle(DEV)
    value = torch.full((1,), np.nan if value_init is None else value_init, device=DEV)
    grad = None
    if want_grad:
        grad = torch.zeros_like(flux) if grad_init is None else grad_init.clone()
    patch = 8 if handle.D == 64 else 16
    argmax = None
    if want_argmax:
        if jitter is None:
            n = ((flux.shape[0] - patch) // stride + 1) * ((flux.shape[1] - patch) // stride + 1)
        else:
            n = int(np.prod([len(b) for b in cases.grid(tuple(flux.shape), patch, stride)]))
        argmax = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    if jitter is not None and not isinstance(jitter[0], torch.Tensor):
        jitter = tuple(torch.from_numpy(np.asarray(j, dtype=np.int64)) for j in jitter)
    handle.prior_fwd_bwd(flux, stride, roll, value, 1.0, grad=grad, grad_coef=coef, marginalize=marginalize, argmax_out=argmax,
                         norm=norm, patch_norm=patch_norm, jitter=jitter, accumulate_value=value_init is not None)
    torch.cuda.synchronize()
    return float(value), None if grad is None else grad.cpu().numpy(), None if argmax is None else argmax.cpu().numpy()


def _check(label, o64, o32, model, flux_np, stride, roll, jitter, marginalize, patch=8, **kwargs):
    """The protocol of the module docstring on one case"""
    shape = flux_np.shape
    total64, d64, arg64, margin = o64
    total32, d32, _, _ = o32
    keep = np.ones(shape, dtype=bool)
    clear = None
    if not marginalize:
        clear = margin >= cases.NEAR_TIE
        assert (~clear).sum() <= 0.01 * clear.size
        keep = ~cases.near_tie_mask(margin, shape, patch, stride, roll, jitter)
    e_ref_value = abs(total32 - total64) / abs(total64)
    e_ref_grad = cases.rel_err(d32, d64, keep)
    g0 = np.random.RandomState(shape[1]).normal(size=shape).astype(np.float32) * np.float32(np.abs(d64).max())
    coef = 0.75
    value, grad, argmax = _evaluate(model, _dev(flux_np), stride, roll, jitter, marginalize, _dev(g0), coef,
                                    want_argmax=not marginalize, **kwargs)
    v0 = 1000.0
    value_acc, _, _ = _evaluate(model, _dev(flux_np), stride, roll, jitter, marginalize, value_init=v0, want_grad=False, **kwargs)
    e_value = abs(value - total64) / abs(total64)
    e_value_acc = abs((value_acc - v0) - total64) / abs(total64)
    expected = g0.astype(np.float64) + coef * d64
    err = np.abs(grad - expected) / np.abs(coef * d64).max()
    e_grad = float(err[keep].max())
    covered = cases.covered_mask(shape, patch, stride, roll, jitter)
    print(f"gmm jitter parity {label} {'lse' if marginalize else 'max'} {shape} stride {stride} roll {roll}: value e_ref "
          f"{e_ref_value:.2e} device {e_value:.2e} accumulated {e_value_acc:.2e} | gradient e_ref {e_ref_grad:.2e} device "
          f"{e_grad:.2e} ({int((~covered).sum())} pixels no patch covers)")
    assert np.abs(d64).max() > 0 and np.isfinite(grad).all() and np.isfinite(value)
    assert e_value <= max(3e-6, 4 * e_ref_value)
    assert e_value_acc <= max(3e-6, 4 * e_ref_value)
    assert e_grad <= max(1e-5, 4 * e_ref_grad)
    # a pixel no patch covers keeps its gradient bits
    assert (d64[~covered] == 0).all() and np.array_equal(grad[~covered], g0[~covered])
    if not marginalize:
        assert np.array_equal(argmax[clear], arg64[clear])


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("index", range(len(cases.CASES)))
@pytest.mark.parametrize("marginalize", [False, True])
def test_prior_matches_the_oracle(golden, model, marginalize, index):
    shape, stride, roll = cases.CASES[index]
    o64 = cases.cached_oracle(golden, index, marginalize, np.float64)
    o32 = cases.cached_oracle(golden, index, marginalize, np.float32)
    _check(f"case {index}", o64, o32, model, cases.case_flux(index), stride, roll, cases.case_draws(index), marginalize)


@pytest.mark.parametrize("index", range(len(cases.CASES_256)))
@pytest.mark.parametrize("marginalize", [False, True])
def test_16x16_patches(golden, model256, marginalize, index):
    shape, stride, roll = cases.CASES_256[index]
    o64 = cases.cached_oracle(golden, index, marginalize, np.float64, table=256)
    o32 = cases.cached_oracle(golden, index, marginalize, np.float32, table=256)
    _check(f"D = 256 case {index}", o64, o32, model256, cases.case_flux(index, 256), stride, roll, cases.case_draws(index, 256),
           marginalize, patch=16)


@pytest.mark.parametrize("name", ["plus", "minus", "alternating", "coincident"])
@pytest.mark.parametrize("marginalize", [False, True])
def test_extreme_draws(golden, model, marginalize, name):
    """Explicit draws on case 0: every jitter +overlap, every jitter -overlap, alternating (neighbouring rows swap places),
    +overlap / 0 (coincident neighbours)"""
    shape, stride, roll = cases.CASES[0]
    o64 = cases.cached_oracle(golden, 0, marginalize, np.float64, extreme=name)
    o32 = cases.cached_oracle(golden, 0, marginalize, np.float32, extreme=name)
    _check(f"extreme {name}", o64, o32, model, cases.case_flux(0), stride, roll, cases.extreme_draws()[name], marginalize)


# ------------------------------------------------------------------------------------------------ 2. norms, patch norm
@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("norm_type", ["asinh", "log"])
def test_image_norms(golden, model, norm_type, marginalize):
    """(37, 41): the scalar path of the adjoint, n applied per staged pixel, n' on the raw flux"""
    index = 7
    shape, stride, roll = cases.CASES[index]
    o64 = cases.cached_oracle(golden, index, marginalize, np.float64, norm_type=norm_type)
    o32 = cases.cached_oracle(golden, index, marginalize, np.float32, norm_type=norm_type)
    _check(norm_type, o64, o32, model, cases.case_flux(index), stride, roll, cases.case_draws(index), marginalize,
           norm=make_norm(norm_type))


def test_standardized_patch_norm(golden, model):
    index = 0
    shape, stride, roll = cases.CASES[index]
    o64 = cases.cached_oracle(golden, index, False, np.float64, patch_norm="std-subtract-mean")
    o32 = cases.cached_oracle(golden, index, False, np.float32, patch_norm="std-subtract-mean")
    _check("std-subtract-mean", o64, o32, model, cases.case_flux(index), stride, roll, cases.case_draws(index), False,
           patch_norm=_std())


# ------------------------------------------------------------------------------------------------ 3. stride = P
@pytest.mark.parametrize("d", [64, 256])
def test_stride_of_a_patch_is_the_plain_pass_bit_for_bit(model, model256, d):
    """Overlap 0: the draws are all 0, S is exactly the contiguous crop flux[:n_y P, :n_x P] -- value, arg-max and the
    accumulated gradient equal `prior_fwd_bwd` on that crop at stride P; pixels outside the crop keep their bits"""
    mdl, patch, shape = (model, 8, (24, 27)) if d == 64 else (model256, 16, (48, 50))
    base_y, base_x = cases.grid(shape, patch, patch)
    n_y, n_x = len(base_y), len(base_x)
    assert (n_y * patch, n_x * patch) in ((16, 24), (32, 48))
    flux_np = np.random.RandomState(shape[0]).gamma(20, size=shape).astype(np.float32)
    g0_np = np.random.RandomState(1).normal(size=shape).astype(np.float32)
    zeros = (np.zeros(n_y, dtype=np.int64), np.zeros(n_x, dtype=np.int64))
    jittered = _evaluate(mdl, _dev(flux_np), patch, None, zeros, False, _dev(g0_np), -0.7, want_argmax=True)
    crop = (slice(0, n_y * patch), slice(0, n_x * patch))
    plain = _evaluate(mdl, _dev(flux_np[crop]), patch, None, None, False, _dev(g0_np[crop]), -0.7, want_argmax=True)
    assert jittered[0] == plain[0] and np.array_equal(jittered[2], plain[2]) and (plain[2] >= 0).all()
    assert np.array_equal(jittered[1][crop], plain[1]) and np.abs(plain[1] - g0_np[crop]).max() > 0
    outside = np.ones(shape, dtype=bool)
    outside[crop] = False
    assert outside.any() and np.array_equal(jittered[1][outside], g0_np[outside])


# ------------------------------------------------------------------------------------------------ 4. untouched pixels
def test_a_zero_sum_under_the_log_norm_keeps_the_gradient_bits(model):
    """A covered pixel whose gathered sum is exactly 0 (coefficient 0: G is zero everywhere) is not written, although n' of
    the log norm is infinite at the zero pixel (5, 7) -- 0 * inf would be a NaN; the patches that hold the pixel are filtered
    by the pass (log 0 = -inf), the value stays finite"""
    shape, stride, roll = cases.CASES[0]
    jitter_np = cases.case_draws(0)
    covered = cases.covered_mask(shape, 8, stride, roll, jitter_np)
    assert covered[5, 7]
    flux_np = cases.case_flux(0).copy()
    flux_np[5, 7] = 0.0
    g0 = _dev(np.random.RandomState(2).normal(size=shape))
    handle = model.handle(DEV)
    value = torch.zeros(1, device=DEV)
    grad = g0.clone()
    jitter = tuple(torch.from_numpy(j) for j in jitter_np)
    handle.prior_fwd_bwd(_dev(flux_np), stride, roll, value, 1.0, grad=grad, grad_coef=0.0, jitter=jitter, norm=make_norm("log"))
    torch.cuda.synchronize()
    assert np.isfinite(float(value)) and np.array_equal(grad.cpu().numpy(), g0.cpu().numpy())
    # (and with a coefficient, on the positive flux, the same call changes the covered pixels and only those)
    handle.prior_fwd_bwd(_dev(cases.case_flux(0)), stride, roll, value, 1.0, grad=grad, grad_coef=1.0, jitter=jitter,
                         norm=make_norm("log"))
    torch.cuda.synchronize()
    changed = grad.cpu().numpy() != g0.cpu().numpy()
    assert changed[covered].mean() > 0.9 and not changed[~covered].any() and np.isfinite(grad.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ 5. draws on the device
def test_device_draws_outside_the_range_are_clamped(model):
    """Device arrays cannot be validated without a synchronisation: a draw outside [-overlap, overlap] is clamped inside the
    kernels -- the run ends clean and equals the run with the clamped draws (host draws outside the range raise)"""
    shape, stride, roll = cases.CASES[0]
    flux = _dev(cases.case_flux(0))
    g0 = _dev(np.random.RandomState(3).normal(size=shape))
    jy, jx = cases.case_draws(0)
    wild_y, wild_x = jy.copy(), jx.copy()
    wild_y[[0, 3]], wild_x[[1, -1]] = (9, -100), (2**30, -(2**30))
    clamped = (np.clip(wild_y, -4, 4), np.clip(wild_x, -4, 4))
    on_device = tuple(torch.from_numpy(j.astype(np.int32)).to(DEV) for j in (wild_y, wild_x))
    got = _evaluate(model, flux, stride, roll, on_device, False, g0, 0.5, want_argmax=True)
    want = _evaluate(model, flux, stride, roll, clamped, False, g0, 0.5, want_argmax=True)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.abs(want[1] - g0.cpu().numpy()).max() > 0
    with pytest.raises(ValueError, match="outside"):
        _evaluate(model, flux, stride, roll, (wild_y, wild_x))
    with pytest.raises(ValueError, match="must hold 7 integer draws"):
        _evaluate(model, flux, stride, roll, (jy[:-1], jx))


# ------------------------------------------------------------------------------------------------ 6. repeatability, forward only
def test_two_runs_give_the_same_bits(model):
    shape, stride, roll = cases.CASES[2]
    flux = _dev(cases.case_flux(2))
    runs = [_evaluate(model, flux, stride, roll, cases.case_draws(2), False, None, 1.0, want_argmax=True) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert np.abs(runs[0][1]).max() > 0


@pytest.mark.parametrize("d", [64, 256])
def test_forward_only_gives_the_same_value_and_touches_no_gradient(model, model256, d):
    mdl, table = (model, 64) if d == 64 else (model256, 256)
    shape, stride, roll = cases.table_of(table)[0][0]
    flux = _dev(cases.case_flux(0, table))
    jitter = cases.case_draws(0, table)
    g0 = _dev(np.random.RandomState(4).normal(size=shape))
    both = _evaluate(mdl, flux, stride, roll, jitter, False, g0, 0.5)
    # (the gradient image G of the call before stays in the handle: a forward-only call must neither need nor change it --
    # the evidence is the third call, which gives the first call's bits again)
    only = _evaluate(mdl, flux, stride, roll, jitter, False, want_grad=False)
    assert only[0] == both[0] and only[1] is None
    again = _evaluate(mdl, flux, stride, roll, jitter, False, g0, 0.5)
    assert again[0] == both[0] and np.array_equal(again[1], both[1])


# ------------------------------------------------------------------------------------------------ 7. autograd
def test_autograd_equals_the_fused_path(model):
    """`prior(flux).backward()`: same value and gradient as `device_fwd_bwd` with the same draw"""
    from jolideco_amd import JitteredGMMPatchPrior

    prior = JitteredGMMPatchPrior(gmm=model, norm=make_norm("asinh"), generator=torch.Generator("cpu").manual_seed(21))
    shape = (40, 44)
    flux = _dev(np.random.RandomState(37).gamma(20, size=shape)).reshape(1, 1, *shape).requires_grad_(True)
    value = prior(flux)
    value.backward()
    roll, (jitter_x, jitter_y) = drawn = prior.last_shifts
    want = cases.draw(torch.Generator("cpu").manual_seed(21), shape)
    assert roll == want[0] and np.array_equal(jitter_y.numpy(), want[1][0]) and np.array_equal(jitter_x.numpy(), want[1][1])
    ref_v, ref_g = torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV)
    prior.device_fwd_bwd(flux.detach(), ref_v, grad=ref_g, coef=1.0, shifts=drawn)
    torch.cuda.synchronize()
    assert float(value.detach()) == float(ref_v)
    assert np.array_equal(flux.grad.cpu().numpy()[0, 0], ref_g.cpu().numpy()) and np.abs(ref_g.cpu().numpy()).max() > 0
    # "draw" takes the shape from the flux and advances the generator as the reference does
    prior.device_fwd_bwd(flux.detach(), ref_v, shifts="draw")
    torch.cuda.synchronize()
    replay = torch.Generator("cpu").manual_seed(21)
    cases.draw(replay, shape)
    want = cases.draw(replay, shape)
    assert prior.last_shifts[0] == want[0] and np.array_equal(prior.last_shifts[1][1].numpy(), want[1][0])


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(golden, model):
    from jolideco_amd import JitteredGMMPatchPrior, _hip
    from jolideco_amd._hip import ptr, stream_ptr

    shape, stride, roll = cases.CASES[0]
    flux = _dev(cases.case_flux(0))
    jitter = cases.case_draws(0)
    before = _evaluate(model, flux, stride, roll, jitter)
    with pytest.raises(ValueError, match="width 41 .* nearest safe width is 40 or 44"):
        _evaluate(model, _dev(np.ones((40, 41))), stride, roll, jitter)
    with pytest.raises(ValueError, match="height 12 .* has no jittered patch"):
        _evaluate(model, _dev(np.ones((12, 44))), stride, roll, jitter)
    with pytest.raises(ValueError, match="whole prior"):
        model.handle(DEV).prior_fwd_bwd(flux, stride, roll, torch.zeros(1, device=DEV), 1.0, jitter=jitter, patch_rows=(0, 2))
    with pytest.raises(ValueError, match="whole prior"):
        model.handle(DEV).prior_fwd_bwd(flux, stride, roll, torch.zeros(1, device=DEV), 1.0, jitter=jitter, subpix=(0.0, 0.0))
    prior = JitteredGMMPatchPrior(gmm=model)
    with pytest.raises(NotImplementedError, match="fused optimizer step"):
        prior.device_fwd_bwd_step(flux, torch.zeros(1, device=DEV), 1.0, None)
    # the library's own refusals (the Python layer refuses the same shapes before it calls): unsafe shape, no patch, stride
    lib, handle = _hip.lib(), model.handle(DEV)
    jy, jx = (torch.zeros(64, dtype=torch.int32, device=DEV) for _ in range(2))
    value = torch.zeros(1, device=DEV)

    def call(f, H, W, s):
        return lib.jd_gmm_prior_jitter_fwd_bwd(handle._handle, ptr(f), H, W, s, 0, 0, ptr(jy), ptr(jx), 0, 1.0, ptr(value), 0, 0.0,
                                               None, None, None, stream_ptr(f.device))

    unsafe = _dev(np.ones((37, 41)))
    assert call(unsafe, 37, 41, 4) == -1 and b"not safe" in lib.jd_last_error()
    assert call(unsafe, 12, 41, 4) == -1 and b"no jittered patch" in lib.jd_last_error()
    assert call(flux, 40, 44, 0) == -1 and call(flux, 40, 44, 9) == -1 and b"stride" in lib.jd_last_error()
    assert call(flux, 40, 44, 3) == -1 and b"not safe" in lib.jd_last_error()  # (below half a patch: no shape is safe)
    with pytest.raises(ValueError, match="stride 3: no image height or width is safe"):
        _evaluate(model, flux, 3, roll, jitter)
    assert lib.jd_gmm_prior_jitter_fwd_bwd(handle._handle, ptr(flux), 40, 44, 4, 0, 0, None, ptr(jx), 0, 1.0, ptr(value), 0, 0.0,
                                           None, None, None, stream_ptr(flux.device)) == -1
    torch.cuda.synchronize()
    after = _evaluate(model, flux, stride, roll, jitter)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    total64 = cases.cached_oracle(golden, 0, False, np.float64)[0]
    assert abs(after[0] - total64) <= 3e-6 * abs(total64)


# ------------------------------------------------------------------------------------------------ 9. fits
def _fit_components(golden):
    from jolideco_amd import JitteredGMMPatchPrior, SpatialFluxComponent
    from image_norm_cases import fixture_gmm

    g = golden("gmm_jitter")
    prior = JitteredGMMPatchPrior(gmm=_model(fixture_gmm(golden, "fit/gmm/")))
    return g, unpack_datasets(g, "fit/data/"), SpatialFluxComponent.from_numpy(flux=g["fit/flux_init"], prior=prior)


def test_sequential_fit_matches_the_reference(golden):
    """6 sequential epochs of a 32 x 32 scene, two observations, default generators, through `MAPDeconvolver.run()`: the
    fixture of the live reference (the tolerance of the sub-pixel fit test); a second run gives the same bits"""
    from jolideco_amd import MAPDeconvolver

    runs = []
    for _ in range(2):
        g, datasets, comp = _fit_components(golden)
        res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False, device=DEV).run(datasets, components=comp)
        runs.append(np.asarray(res.flux_total).copy())
        err = rel_linf(res.flux_total, g["fit/flux_final"])
        print(f"gmm jitter fit: flux rel Linf {err:.2e}")
        assert err < 1e-5
        np.testing.assert_allclose(res.trace_loss["total"], g["fit/trace/total"], rtol=1e-4)
    assert np.array_equal(runs[0], runs[1])


def test_session_runs_by_value_epochs(golden):
    from jolideco_amd import MAPDeconvolver

    _, datasets, comp = _fit_components(golden)
    session = MAPDeconvolver(n_epochs=3, display_progress=False, device=DEV, fit_mode="joint").session(datasets, components=comp)
    assert session.has_jitter_patches and not session._planned_capable()
    assert not session._fuse_step(session.states[0], session.priors[0])
    for _ in range(3):
        session.epoch()
    torch.cuda.synchronize()
    assert session.graph_policy.startswith("by value") and "JitteredGMMPatchPrior" in session.graph_policy and not session._graphs
    roll, (jitter_x, jitter_y) = session.priors[0].last_shifts
    assert len(jitter_x) == len(jitter_y) == 5 and np.isfinite(session.states[0].flux_cur.cpu().numpy()).all()

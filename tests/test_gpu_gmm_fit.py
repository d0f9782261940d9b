"""GPU: the EM fit of a Gaussian mixture (csrc/gmm_fit.hip, `GaussianMixtureModel.fit` / `fit_images`) against the
float64 restatement of scikit-learn's EM step (tests/gmm_fit_cases.py, pinned by tests/golden/gmm_fit.npz).

Bounds: per quantity (weights, means, covariances, lower bound) max(FLOOR, 4 e_ref), where e_ref is the error of the same
restatement run in float32 against its float64 run and 4 the project's factor for an equally rounded evaluation in
another order (tests/test_gpu_image_norm.py).  The errors are `gmm_fit_cases.errors`: relative to the largest entry of
the quantity, the covariances relative to the second moments about the start means.  The floors cover the cases where
e_ref is no measure of the device's rounding -- a single patch, where the float32 restatement subtracts the patch from
itself and is exact -- and are at most twice the largest device error of their quantity measured on an MI355X (weights
1.0e-6, means 8.0e-6, covariances 6.5e-6, lower bound 2.5e-8); the measured errors and e_ref of every case are in
profiles/gmm_fit/README.md.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import gmm_fit_cases as cases
from conftest import patch_cover_mask
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 2.4e-7 = 4 x 2^-24: the device gets the means, factors and constants rounded to float32, so no result is closer to the
# float64 reference than a few float32 roundings; the lower bound is a mean over the patches and does better
FLOORS = {"weights": 2.4e-7, "means": 2.4e-7, "covariances": 2.4e-7, "lower_bound": 5e-8}


def bounds_of(e_ref):
    return {name: max(FLOORS[name], 4 * e_ref[name]) for name in FLOORS}


def check(label, got, ref64, ref32, start_means):
    e_ref, err = cases.errors(ref32, ref64, start_means), cases.errors(got, ref64, start_means)
    bound = bounds_of(e_ref)
    print(f"gmm fit {label}: " + " | ".join(f"{name} e_ref {e_ref[name]:.2e} device {err[name]:.2e} bound {bound[name]:.2e}" for name in FLOORS))
    for part in got:
        assert np.isfinite(np.asarray(part)).all()
    for name in FLOORS:
        assert err[name] <= bound[name], f"{label}: {name} error {err[name]:.2e} > {bound[name]:.2e}"
    return bound


def device_step(x, weights, means, covariances, reg=cases.REG_COVAR, max_blocks=0):
    """The product's path of one step: the device sums and the host finish -- (weights, means, covariances, [bound])"""
    from jolideco_amd.ops import GmmFitHandle
    from jolideco_amd.priors.patches.gmm import em_step

    handle = GmmFitHandle(x.shape[1], len(weights), DEV, max_blocks)
    x_dev = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).to(DEV)
    new_means, new_cov, new_weights, bound, _ = em_step(handle, x_dev, np.array(means), np.array(covariances), np.array(weights), reg)
    handle.close()
    return new_weights, new_means, new_cov, np.array([bound])


def raw_sums(handle, x_dev, weights, means, covariances):
    """What the kernel wrote for a start: the four arrays of `GmmFitHandle.step`"""
    from jolideco_amd.priors.patches.gmm import _upload
    from jolideco_amd.utils.numpy import compute_precision_cholesky

    K, D = means.shape
    prec = compute_precision_cholesky(covariances).astype(np.float32)
    const = np.log(weights) + np.log(np.diagonal(prec, axis1=1, axis2=2).astype(np.float64)).sum(axis=1) - 0.5 * D * np.log(2 * np.pi)
    return handle.step(x_dev, _upload(means, DEV), _upload(prec, DEV), _upload(const, DEV))


# ------------------------------------------------------------------------------------------- 1. one step against float64
# (by default 17 blocks share the 4099 patches; max_blocks = 1: one block walks them in three chunks of at most 2048 and
# adds to its float64 partial sums twice)
@pytest.mark.parametrize("case, max_blocks", [(c, 0) for c in cases.STEP_CASES] + [((64, 17, 4099), 1)],
                         ids=lambda v: cases.case_name(*v) if isinstance(v, tuple) else f"blocks{v}")
def test_one_step_matches_float64(case, max_blocks):
    x, weights, means, covariances = cases.case_inputs(*case)
    ref = cases.reference(*case)
    got = device_step(x, weights, means, covariances, max_blocks=max_blocks)
    check(f"{cases.case_name(*case)} max_blocks {max_blocks}", got, ref["float64"], ref["float32"], means)


# ------------------------------------------------------------------------------------------------ 2. far-apart components
def test_far_apart_components_do_not_mix():
    rs = np.random.RandomState(77)
    D, sizes = 64, (150, 107)
    centre = rs.standard_normal(D) * 3.0
    x = np.concatenate([sign * centre + 0.7 * rs.standard_normal((m, D)) for sign, m in zip((1.0, -1.0), sizes)]).astype(np.float32)
    n = x.shape[0]
    means = np.stack([centre, -centre]) + 0.05 * rs.standard_normal((2, D))
    a = rs.standard_normal((2, D, D)) / np.sqrt(D)
    covariances = 0.3 * np.einsum("kij,klj->kil", a, a) + 0.3 * np.eye(D)[None]
    weights = np.array([0.4, 0.6])
    l = cases.log_prob(x.astype(np.float64), weights, means, covariances)
    assert np.abs(l[:, 0] - l[:, 1]).min() >= 1e3  # the smaller l is at least 1e3 below the larger, for every patch
    joint = device_step(x, weights, means, covariances)
    alone, at = [], 0
    for k, m in enumerate(sizes):
        alone.append(device_step(x[at:at + m], np.ones(1), means[k:k + 1], covariances[k:k + 1]))
        at += m
    expected = (np.array(sizes) / n, np.concatenate([r[1] for r in alone]), np.concatenate([r[2] for r in alone]),
                np.array([sum(m * (r[3][0] + np.log(w)) for m, r, w in zip(sizes, alone, weights)) / n]))
    ref64, ref32 = (cases.em_steps(x, weights, means, covariances, 1, dtype=d) for d in ("float64", "float32"))
    check("far apart, against float64", joint, ref64, ref32, means)
    check("far apart, against the clusters alone", joint, expected, tuple(np.asarray(p) + (np.asarray(q) - np.asarray(r))
                                                                          for p, q, r in zip(expected, ref32, ref64)), means)


# ------------------------------------------------------------------------------------- 3. / 4. identical bits
def test_two_runs_and_an_unaligned_input_give_the_same_bits():
    from jolideco_amd.ops import GmmFitHandle

    case = (64, 17, 4099)
    x, weights, means, covariances = cases.case_inputs(*case)
    n, D = x.shape
    buffer = torch.zeros(n * D + 8, device=DEV)
    aligned, unaligned = buffer[4:4 + n * D].view(n, D), buffer[1:1 + n * D].view(n, D)
    assert aligned.data_ptr() % 16 == 0 and unaligned.data_ptr() % 16 == 4 and unaligned.is_contiguous()
    handle = GmmFitHandle(D, case[1], DEV)
    aligned.copy_(torch.from_numpy(np.array(x)))
    first = raw_sums(handle, aligned, weights, means, covariances)
    second = raw_sums(handle, aligned, weights, means, covariances)
    fresh = raw_sums(GmmFitHandle(D, case[1], DEV), aligned.clone(), weights, means, covariances)
    buffer.zero_()
    unaligned.copy_(torch.from_numpy(np.array(x)))
    shifted = raw_sums(handle, unaligned, weights, means, covariances)
    assert np.abs(first[2]).max() > 0 and np.isfinite(first[3])
    for other in (second, fresh, shifted):
        for a, b in zip(first, other):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------ 5. five iterations
@pytest.mark.parametrize("reg", cases.FIVE_REGS)
def test_five_iterations_follow_the_float64_fit(golden, reg):
    from jolideco_amd.priors.patches import GaussianMixtureModel

    fixture, name = golden("gmm_fit"), f"five_reg{reg:g}"
    x, weights, means, covariances = cases.case_inputs(*cases.FIVE_CASE)
    model = GaussianMixtureModel.fit(torch.from_numpy(np.array(x)).to(DEV), means_init=means, covariances_init=covariances,
                                     weights_init=weights, n_iter=cases.FIVE_STEPS, tol=0.0, reg_covar=reg)
    info = model.fit_info
    assert info["n_iter"] == cases.FIVE_STEPS and not info["converged"] and model.n_components == 3
    ref = cases.reference(*cases.FIVE_CASE, cases.FIVE_STEPS, reg)
    before_last = cases.reference(*cases.FIVE_CASE, cases.FIVE_STEPS - 1, reg)["float64"][1]
    got = (info["weights"], info["means"], info["covariances"], np.array(info["lower_bounds"]))
    bound = check(f"five steps reg {reg:g}", got, ref["float64"], ref["float32"], before_last)
    # ... and against scikit-learn's own five steps where the fixture holds them
    assert cases.rel_max(got[0], fixture[f"{name}/weights"]) <= bound["weights"]
    assert cases.rel_max(got[1], fixture[f"{name}/means"]) <= bound["means"]
    assert cases.rel_max(got[3], fixture[f"{name}/lower_bounds"]) <= bound["lower_bound"]
    delta = ref["float64"][1] - before_last
    scale = np.abs(ref["float64"][2] + delta[:, :, None] * delta[:, None, :]).max()
    assert cases.rel_max(cases.cov_sample(got[2]), fixture[f"{name}/covariances_sample"], scale=scale) <= bound["covariances"]
    steps = np.diff(got[3])
    print(f"five steps reg {reg:g}: lower bounds {got[3]}, smallest increase {steps.min():.3e}")
    assert steps.min() >= -bound["lower_bound"] * np.abs(got[3]).max()
    # the model holds the float32 roundings of the result
    assert np.array_equal(model.means_numpy, info["means"].astype(np.float32))


# --------------------------------------------------------------------------------------------------------- 6. use as a prior
def _oracle_prior(flux_np, arrays, meta_stride, stride, marginalize, dtype):
    """sum over the patches of the prior's per-patch value, its gradient, and in max mode the margin between the two
    best components (oracle/cpu_ref, as tests/image_norm_cases.oracle evaluates it)"""
    with cpu_ref.precision(dtype):
        gmm = cpu_ref.GMM.from_numpy(*arrays, stride=meta_stride)
        flux = cpu_ref._tensor(flux_np[np.newaxis, np.newaxis]).requires_grad_(True)
        loglike = cpu_ref.gmm_patch_log_like(flux, gmm, stride, None)
        top = torch.topk(loglike, 2, dim=1).values
        values = torch.logsumexp(loglike, dim=1) if marginalize else top[:, 0]
        total = torch.sum(values)
        total.backward()
        return float(total.detach()), flux.grad.numpy()[0, 0].astype(np.float64), (top[:, 0] - top[:, 1]).detach().numpy()


@pytest.fixture(scope="module")
def fitted():
    from jolideco_amd.priors.patches import GaussianMixtureModel

    image = torch.from_numpy(np.random.RandomState(5).gamma(20, size=(96, 96)).astype(np.float32)).to(DEV)
    return GaussianMixtureModel.fit_images(image, stride=2, n_components=4)


@pytest.mark.parametrize("marginalize", [False, True])
def test_a_fitted_mixture_serves_as_a_prior(fitted, marginalize, tmp_path):
    from jolideco_amd import GMMPatchPrior
    from jolideco_amd.priors.patches import GaussianMixtureModel

    info = fitted.fit_info
    assert info["converged"] and 1 < info["n_iter"] < 100 and fitted.meta.stride == 2 and fitted.n_components == 4
    assert np.all(np.diff(info["lower_bounds"]) > -1e-4)
    prior = GMMPatchPrior(gmm=fitted, cycle_spin=False, marginalize=marginalize)
    shape = (40, 44)
    flux_np = np.random.RandomState(6).gamma(20, size=shape).astype(np.float32)
    flux, value, grad = torch.from_numpy(flux_np).to(DEV), torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV)
    prior.device_fwd_bwd(flux, value, grad=grad, coef=1.0, shifts=None)
    torch.cuda.synchronize()
    scale = prior.log_like_weight / flux.numel()
    value, grad = float(value) / scale, grad.cpu().numpy().astype(np.float64) / scale
    arrays = (info["means"], info["covariances"], info["weights"])
    total64, d64, margin = _oracle_prior(flux_np, arrays, 2, prior.stride, marginalize, np.float64)
    total32, d32, _ = _oracle_prior(flux_np, arrays, 2, prior.stride, marginalize, np.float32)
    keep = np.ones(shape, dtype=bool)
    if not marginalize:  # a near-tie may resolve differently under another summation order: those patches are left out
        keep = ~patch_cover_mask(np.flatnonzero(margin <= 1e-3), shape, prior.stride, None)
        assert keep.mean() > 0.9
    norm = np.abs(d64).max()
    e_ref_value, e_ref_grad = abs(total32 - total64) / abs(total64), np.abs(d32 - d64)[keep].max() / norm
    e_value, e_grad = abs(value - total64) / abs(total64), np.abs(grad - d64)[keep].max() / norm
    print(f"fitted prior {'lse' if marginalize else 'max'}: value e_ref {e_ref_value:.2e} device {e_value:.2e} | gradient e_ref "
          f"{e_ref_grad:.2e} device {e_grad:.2e}")
    assert np.isfinite(value) and np.isfinite(grad).all() and norm > 0
    assert e_value <= max(3e-6, 4 * e_ref_value)
    assert e_grad <= max(1e-5, 4 * e_ref_grad)
    # ... and goes through write / read unchanged in kind
    path = tmp_path / "fitted.fits"
    fitted.write(path)
    again = GaussianMixtureModel.read(path, format="table")
    assert np.array_equal(again.means_numpy, fitted.means_numpy) and type(again.meta.patch_norm) is type(fitted.meta.patch_norm)


def test_fit_images_drops_patches_the_prior_would_drop():
    from jolideco_amd.priors.patches import GaussianMixtureModel

    image_np = np.random.RandomState(5).gamma(20, size=(96, 96)).astype(np.float32)
    clean = GaussianMixtureModel.fit_images(torch.from_numpy(image_np[:, :40].copy()).to(DEV), stride=2, n_components=2, n_iter=3)
    image_np[:, 40:] = np.nan
    image_np[:, 60:] = -1e6
    dirty = GaussianMixtureModel.fit_images(torch.from_numpy(image_np).to(DEV), stride=2, n_components=2, n_iter=3)
    assert np.array_equal(clean.means_numpy, dirty.means_numpy) and np.isfinite(dirty.covariances_numpy).all()


# ------------------------------------------------------------------------------------------------------ 7. starved component
def test_a_starved_component_is_named_and_the_handle_survives():
    from jolideco_amd.priors.patches import GaussianMixtureModel
    from jolideco_amd.priors.patches.gmm import _FIT_HANDLES

    case = (64, 3, 4099)
    x, weights, means, covariances = cases.case_inputs(*case)
    x_dev = torch.from_numpy(np.array(x)).to(DEV)
    far = np.array(means)
    far[2] += 1000.0
    with pytest.raises(ValueError, match="component 2 is starved"):
        GaussianMixtureModel.fit(x_dev, means_init=far, covariances_init=covariances, weights_init=weights, n_iter=3)
    handles = dict(_FIT_HANDLES)
    model = GaussianMixtureModel.fit(x_dev, means_init=means, covariances_init=covariances, weights_init=weights, n_iter=1, tol=0.0)
    assert dict(_FIT_HANDLES) == handles and len(handles) >= 1  # the same work space served both
    ref = cases.reference(*case)
    info = model.fit_info
    check("after a starved fit", (info["weights"], info["means"], info["covariances"], np.array(info["lower_bounds"])),
          ref["float64"], ref["float32"], means)


def test_the_random_start_is_deterministic():
    from jolideco_amd.priors.patches import GaussianMixtureModel

    x_dev = torch.from_numpy(np.array(cases.case_inputs(64, 5, 1000)[0])).to(DEV)
    a = GaussianMixtureModel.fit(x_dev, 3, n_iter=2, random_state=4)
    b = GaussianMixtureModel.fit(x_dev, 3, n_iter=2, random_state=4)
    c = GaussianMixtureModel.fit(x_dev, 3, n_iter=2, random_state=5)
    assert np.array_equal(a.covariances_numpy, b.covariances_numpy) and a.fit_info["lower_bounds"] == b.fit_info["lower_bounds"]
    assert not np.array_equal(a.means_numpy, c.means_numpy) and np.isfinite(c.covariances_numpy).all()

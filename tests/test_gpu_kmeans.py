"""GPU: the k-means start of the mixture fit -- one Lloyd step (csrc/kmeans.hip), `kmeans`, the hard-label moments
(`jd_gmm_fit_step_labels`) and `GaussianMixtureModel.fit(init_params="kmeans")` -- against the float64 restatement of
tests/kmeans_cases.py.

Labels are compared outside the ambiguous set (margin of the two smallest float64 scores <= tau_n, kmeans_cases.tau), which
is empty for the separated cases and at most 1 % for the overlapping ones.  Counts are exact; the cluster sums agree with
float64 sums formed with the device's own labels to 1e-12 of the largest entry; the inertia error against float64 is at
most max(4 e_ref, 1e-6) (the rule of tests/test_multiscale_golden.py).  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import gmm_fit_cases as fit_cases
import kmeans_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_CASES = [(*c, "separated") for c in cases.STEP_CASES] + [(*c, "overlap") for c in cases.OVERLAP_CASES]


def device_step(x, centres, old_labels=None, handle=None, max_blocks=0):
    """(labels, counts, sums, inertia, changed, unassigned) of one device step"""
    from jolideco_amd.ops import KMeansHandle

    K, D = centres.shape
    own = handle is None
    handle = KMeansHandle(D, K, DEV, max_blocks) if own else handle
    x_dev = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).to(DEV)
    labels = torch.full((x_dev.shape[0],), -1, dtype=torch.int32, device=DEV)
    if old_labels is not None:
        labels.copy_(torch.from_numpy(np.asarray(old_labels, dtype=np.int32)))
    out = handle.step(x_dev, torch.from_numpy(np.array(centres, dtype=np.float32)).to(DEV), labels)
    if own:
        handle.close()
    return (labels.cpu().numpy(), *out)


# ---------------------------------------------------------------------------------------- 1. one step against float64
# (max_blocks = 1: one block walks all 4099 patches and all 33 tiles)
@pytest.mark.parametrize("case, max_blocks", [(c, 0) for c in ALL_CASES] + [((64, 17, 4099, "overlap"), 1)],
                         ids=lambda v: cases.case_name(*v) if isinstance(v, tuple) else f"blocks{v}")
def test_one_step_matches_float64(case, max_blocks):
    x, centres = cases.case_inputs(*case)
    ref = cases.reference(*case)
    ref64, ambiguous = ref["float64"], ref["ambiguous"]
    labels, counts, sums, inertia, changed, unassigned = device_step(x, centres, max_blocks=max_blocks)
    differ = labels != ref64["labels"]
    e_ref = abs(ref["float32"]["inertia"] - ref64["inertia"]) / ref64["inertia"]
    err = abs(inertia - ref64["inertia"]) / ref64["inertia"]
    own_counts, own_sums = cases.cluster_sums(x, labels, case[1])
    e_sums = np.abs(sums - own_sums).max() / np.abs(own_sums).max()
    print(f"kmeans {cases.case_name(*case)} max_blocks {max_blocks}: ambiguous {ambiguous.sum()} of {x.shape[0]}, labels that differ "
          f"{differ.sum()} (decided: {differ[~ambiguous].sum()}) | sums {e_sums:.2e} | inertia e_ref {e_ref:.2e} device {err:.2e}")
    if case[3] == "separated":
        assert not ambiguous.any()
    else:
        assert ambiguous.mean() <= cases.AMBIGUOUS_MAX
    assert not differ[~ambiguous].any()
    assert labels.min() >= 0 and labels.max() < case[1] and unassigned == 0 and changed == x.shape[0]
    assert np.array_equal(counts, own_counts) and counts.sum() == x.shape[0]
    if not differ.any():
        assert np.array_equal(counts, ref64["counts"])
    assert e_sums <= 1e-12
    assert err <= max(4 * e_ref, 1e-6)


# ------------------------------------------------------------------------------------------------------ 2. special inputs
def test_identical_centres_go_to_the_lower_index():
    x, centres = cases.case_inputs(64, 17, 4099)
    doubled = np.array(centres)
    doubled[9] = doubled[4]
    doubled[16] = doubled[4]
    labels, counts, sums, *_ = device_step(x, doubled)
    ref = cases.lloyd_step(x, doubled)
    assert np.array_equal(labels, ref["labels"]) and counts[4] > 0 and counts[9] == 0 and counts[16] == 0
    assert not sums[9].any() and not sums[16].any() and np.array_equal(counts, ref["counts"])


def test_a_far_centre_stays_empty_and_keeps_its_place():
    from jolideco_amd.priors.patches import kmeans

    x, centres = cases.case_inputs(64, 3, 33)
    far = np.array(centres)
    far[1] = 1000.0
    result = kmeans(torch.from_numpy(np.array(x)).to(DEV), 3, centres_init=far, max_iter=4)
    assert result.counts[1] == 0 and np.array_equal(result.centres[1], far[1].astype(np.float64))
    assert result.converged and result.counts.sum() == 33 and not (result.labels == 1).any()
    assert not np.array_equal(result.centres[0], far[0].astype(np.float64))


def test_a_patch_with_a_nan_is_left_out():
    x, centres = cases.case_inputs(64, 17, 4099)
    dirty = np.array(x)
    rows = [0, 130, 4098]
    dirty[0, 5] = np.nan
    dirty[130, 63] = np.inf
    dirty[4098, 0] = -np.inf
    labels, counts, sums, inertia, changed, unassigned = device_step(dirty, centres)
    clean = np.delete(np.array(x), rows, axis=0)
    ref_labels, ref_counts, ref_sums, ref_inertia, *_ = device_step(clean, centres)
    assert unassigned == 3 and (labels[rows] == -1).all() and np.array_equal(np.delete(labels, rows), ref_labels)
    assert np.array_equal(counts, ref_counts) and np.isfinite(sums).all() and np.isfinite(inertia)
    assert np.abs(sums - ref_sums).max() <= 1e-12 * np.abs(ref_sums).max()
    assert abs(inertia - ref_inertia) <= 1e-12 * ref_inertia
    assert changed == 4099 - 3  # the three hold -1 as before


def test_changed_counts_against_the_labels_passed_in():
    x, centres = cases.case_inputs(64, 17, 4099)
    ref = cases.reference(64, 17, 4099)["float64"]
    old = ref["labels"].copy()
    assert device_step(x, centres, old_labels=old)[4] == 0
    old[[0, 17, 2048, 4098]] = [-1, 99, (old[2048] + 1) % 17, (old[4098] + 3) % 17]
    labels, *_, changed, _ = device_step(x, centres, old_labels=old)
    assert changed == 4 and np.array_equal(labels, ref["labels"])


def test_two_calls_give_the_same_bits():
    from jolideco_amd.ops import KMeansHandle

    case = (64, 17, 4099, "overlap")
    x, centres = cases.case_inputs(*case)
    handle = KMeansHandle(64, 17, DEV)
    x_dev = torch.from_numpy(np.array(x)).to(DEV)
    first = device_step(x_dev, centres, handle=handle)
    second = device_step(x_dev, centres, handle=handle)
    fresh = device_step(x_dev.clone(), centres)
    assert np.abs(first[2]).max() > 0
    for other in (second, fresh):
        for a, b in zip(first, other):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------- 3. several iterations
def test_five_iterations_follow_the_float64_run():
    from jolideco_amd.ops import KMeansHandle
    from jolideco_amd.priors.patches import kmeans

    x, init = cases.five_inputs()
    steps = cases.five_reference()
    x_dev = torch.from_numpy(np.array(x)).to(DEV)
    handle = KMeansHandle(64, cases.FIVE_CASE[1], DEV)
    centres, old = np.asarray(init, dtype=np.float64), None
    for i, step in enumerate(steps):  # the loop of `kmeans`, a step at a time
        labels, counts, sums, inertia, changed, _ = device_step(x_dev, centres, old_labels=old, handle=handle)
        assert np.array_equal(labels, step["labels"]) and changed == step["changed"], f"iteration {i}"
        filled = counts > 0
        centres = centres.copy()
        centres[filled] = (sums[filled] / counts[filled, None]).astype(np.float32).astype(np.float64)
        ulp = np.spacing(np.abs(step["centres"]).astype(np.float32)).astype(np.float64)
        print(f"kmeans five steps, iteration {i}: changed {changed}, centres off by {(np.abs(centres - step['centres']) / ulp).max():.2f} ulp")
        assert (np.abs(centres - step["centres"]) <= ulp).all()
        old = labels
    result = kmeans(x_dev, cases.FIVE_CASE[1], centres_init=init, max_iter=cases.FIVE_STEPS)
    assert result.n_iter == 5 and result.converged and np.array_equal(result.labels.cpu().numpy(), steps[-1]["labels"])
    assert np.array_equal(result.counts, steps[-1]["counts"]) and len(result.inertia) == 5
    assert (np.abs(result.centres - steps[-2]["centres"]) <= np.spacing(np.abs(steps[-2]["centres"]).astype(np.float32))).all()
    assert np.all(np.diff(result.inertia) <= 0)
    short = kmeans(x_dev, cases.FIVE_CASE[1], centres_init=init, max_iter=3)
    assert short.n_iter == 3 and not short.converged and np.array_equal(short.labels.cpu().numpy(), steps[2]["labels"])


def test_kmeans_seeds_itself_and_is_deterministic():
    from jolideco_amd.priors.patches import kmeans

    x, _ = cases.case_inputs(64, 17, 4099)
    x_dev = torch.from_numpy(np.array(x)).to(DEV)
    a = kmeans(x_dev, 17, random_state=3)
    b = kmeans(x_dev, 17, random_state=3)
    c = kmeans(x_dev, 17, random_state=4, n_seed=500)
    assert a.converged and np.array_equal(a.centres, b.centres) and a.inertia == b.inertia
    assert torch.equal(a.labels, b.labels) and a.labels.dtype == torch.int32 and a.labels.is_cuda
    assert a.counts.sum() == 4099 and c.counts.sum() == 4099 and a.centres.dtype == np.float64
    assert np.array_equal(a.centres, a.centres.astype(np.float32).astype(np.float64))
    # seventeen far-apart blobs: k-means++ finds one seed per blob, and Lloyd stays there
    truth = cases.reference(64, 17, 4099)["float64"]
    assert sorted(a.counts.tolist()) == sorted(truth["counts"].tolist())


# ------------------------------------------------------------------------------------------------ 4. hard-label moments
def hard_moments(x, means32, labels, K):
    x64 = np.asarray(x, dtype=np.float64)
    D = x64.shape[1]
    s0, s1, s2 = np.zeros(K), np.zeros((K, D)), np.zeros((K, D, D))
    for k in range(K):
        d = x64[labels == k] - means32[k].astype(np.float64)
        s0[k], s1[k], s2[k] = d.shape[0], d.sum(axis=0), d.T @ d
    return s0, s1, s2


@pytest.mark.parametrize("case", fit_cases.STEP_CASES, ids=lambda c: fit_cases.case_name(*c))
def test_hard_label_moments_match_float64(case):
    """The bounds of tests/test_gpu_gmm_fit.py for the soft step at the same cases: the M-step finished from the device's
    sums against the float64 M-step from float64 sums with the same labels, per quantity max(floor, 4 e_ref) with e_ref
    the error of the float32 restatement of the soft step of the case."""
    from test_gpu_gmm_fit import bounds_of

    from jolideco_amd.ops import GmmFitHandle
    from jolideco_amd.priors.patches.gmm import em_m_step

    D, K, n = case
    x, weights, means, covariances = fit_cases.case_inputs(*case)
    ref = fit_cases.reference(*case)
    bound = bounds_of(fit_cases.errors(ref["float32"], ref["float64"], means))
    means32 = np.asarray(means).astype(np.float32)
    labels = cases.lloyd_step(x, means32)["labels"]
    with_bad = labels.copy()
    x_dev = torch.from_numpy(np.array(x)).to(DEV)
    handle = GmmFitHandle(D, K, DEV)
    got = handle.step_labels(x_dev, torch.from_numpy(means32).to(DEV), torch.from_numpy(labels).to(DEV))
    expect = hard_moments(x, means32, labels, K)
    assert np.array_equal(got[0], expect[0])
    filled = expect[0] > 0
    fin_got = em_m_step(means32.astype(np.float64)[filled], got[0][filled], got[1][filled], got[2][filled], n, fit_cases.REG_COVAR)
    fin_ref = em_m_step(means32.astype(np.float64)[filled], *(e[filled] for e in expect), n, fit_cases.REG_COVAR)
    err = fit_cases.errors((fin_got[2], fin_got[0], fin_got[1], np.zeros(1)), (fin_ref[2], fin_ref[0], fin_ref[1], np.ones(1)),
                           means32[filled])
    print(f"hard moments {fit_cases.case_name(*case)}: " + " | ".join(f"{q} device {err[q]:.2e} bound {bound[q]:.2e}"
                                                                       for q in ("weights", "means", "covariances")))
    for q in ("weights", "means", "covariances"):
        assert err[q] <= bound[q]
    # labels of -1 and K change no sum: the device's own sums over the other patches (the patches are centred in float32
    # before they are summed, so sums of the same patches agree to float64 rounding, sums against float64 only to float32's)
    if n >= 4:
        with_bad[[0, n - 1]] = [-1, K]
        means_dev = torch.from_numpy(means32).to(DEV)
        again = handle.step_labels(x_dev, means_dev, torch.from_numpy(with_bad).to(DEV))
        kept = handle.step_labels(x_dev[1:n - 1].contiguous(), means_dev, torch.from_numpy(labels[1:n - 1].copy()).to(DEV))
        assert np.array_equal(again[0], kept[0]) and again[0].sum() == (labels[1:n - 1] >= 0).sum()
        for a, b in zip(again[1:], kept[1:]):
            assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)
        wild = np.full(n, 2**31 - 1, dtype=np.int32)
        wild[::2] = -(2**31)
        none = handle.step_labels(x_dev, torch.from_numpy(means32).to(DEV), torch.from_numpy(wild).to(DEV))
        assert not none[0].any() and not none[1].any() and not none[2].any()
    handle.close()


# -------------------------------------------------------------------------------------------------- 5. the start of the fit
@pytest.fixture(scope="module")
def blobs():
    """600 patches each of four well separated clusters with full-rank scatter: every cluster can carry a covariance"""
    rs = np.random.RandomState(21)
    centres = rs.standard_normal((4, 64)) * 3.0
    label = np.repeat(np.arange(4), 600)
    x = (centres[label] + rs.standard_normal((label.size, 64)) * np.linspace(0.3, 1.0, 64)[None, :]).astype(np.float32)
    return torch.from_numpy(x[rs.permutation(label.size)]).to(DEV)


def test_fit_from_the_kmeans_start_equals_the_fit_from_the_start_it_reports(blobs):
    from jolideco_amd.priors.patches import GaussianMixtureModel

    a = GaussianMixtureModel.fit(blobs, 4, init_params="kmeans", n_iter=3, tol=0.0, random_state=2)
    start = a.fit_info["kmeans"]
    assert set(start) >= {"inertia", "n_iter", "converged", "counts"} and start["converged"] and start["n_iter"] == len(start["inertia"])
    assert sorted(start["counts"].tolist()) == [600.0] * 4 and abs(start["weights"].sum() - 1) < 1e-12
    b = GaussianMixtureModel.fit(blobs, means_init=start["means"], covariances_init=start["covariances"],
                                 weights_init=start["weights"], n_iter=3, tol=0.0)
    assert "kmeans" not in b.fit_info
    for key in ("means", "covariances", "weights"):
        assert np.array_equal(a.fit_info[key], b.fit_info[key])
    assert a.fit_info["lower_bounds"] == b.fit_info["lower_bounds"] and np.array_equal(a.covariances_numpy, b.covariances_numpy)
    # the start is the clusters' own statistics: scikit-learn's M-step from one-hot responsibilities
    # (the device centres the patches on the float32 centres in float32: d carries a relative rounding of 2^-24, the
    # mean of the d at most 2^-24 max |d|, a product d_i d_j at most 2^-23 max |d|^2; twice that is allowed)
    from jolideco_amd.priors.patches import kmeans

    x = blobs.cpu().numpy().astype(np.float64)
    clusters = kmeans(blobs, 4, random_state=2)
    labels = clusters.labels.cpu().numpy()
    for k in range(4):
        member = x[labels == k]
        d_max = np.abs(member - clusters.centres[k]).max()
        cov = np.cov(member.T, bias=True) + 1e-6 * np.eye(64)
        e_mean, e_cov = np.abs(start["means"][k] - member.mean(axis=0)).max(), np.abs(start["covariances"][k] - cov).max()
        print(f"kmeans start, cluster {k}: mean off by {e_mean:.2e} (allowed {2**-23 * d_max:.2e}), covariance by {e_cov:.2e} "
              f"(allowed {2**-22 * d_max**2:.2e})")
        assert e_mean <= 2**-23 * d_max and e_cov <= 2**-22 * d_max**2


def test_the_default_start_is_unchanged(blobs):
    from jolideco_amd.priors.patches import GaussianMixtureModel
    from jolideco_amd.priors.patches.gmm import random_start

    means, covariances, weights = random_start(blobs, 4, 1e-6, 7)
    explicit = GaussianMixtureModel.fit(blobs, means_init=means, covariances_init=covariances, weights_init=weights, n_iter=2, tol=0.0)
    for kwargs in ({}, {"init_params": "random-patches"}):
        default = GaussianMixtureModel.fit(blobs, 4, n_iter=2, tol=0.0, random_state=7, **kwargs)
        assert "kmeans" not in default.fit_info
        for key in ("means", "covariances", "weights"):
            assert np.array_equal(default.fit_info[key], explicit.fit_info[key])
        assert default.fit_info["lower_bounds"] == explicit.fit_info["lower_bounds"]


def test_a_starved_cluster_is_named_before_em():
    from jolideco_amd.priors.patches import GaussianMixtureModel

    x, _ = cases.case_inputs(64, 17, 4099)
    x_dev = torch.from_numpy(np.array(x[:300])).to(DEV)  # 17 blobs of about 18 patches: no cluster reaches D = 64
    with pytest.raises(ValueError, match="starved by the k-means start"):
        GaussianMixtureModel.fit(x_dev, 17, init_params="kmeans")


def test_fit_images_passes_the_start_through():
    from jolideco_amd import GMMPatchPrior
    from jolideco_amd.priors.patches import GaussianMixtureModel

    image = torch.from_numpy(np.random.RandomState(5).gamma(20, size=(64, 64)).astype(np.float32)).to(DEV)
    model = GaussianMixtureModel.fit_images(image, stride=1, n_components=3, init_params="kmeans", kmeans_iter=20, n_iter=5)
    info = model.fit_info
    assert "kmeans" in info and info["kmeans"]["n_iter"] <= 20 and info["kmeans"]["counts"].sum() == 57 * 57
    assert model.n_components == 3 and np.isfinite(model.covariances_numpy).all() and np.all(np.diff(info["lower_bounds"]) > -1e-4)
    prior = GMMPatchPrior(gmm=model, cycle_spin=False)
    flux, value, grad = image[:40, :44].contiguous(), torch.zeros(1, device=DEV), torch.zeros((40, 44), device=DEV)
    prior.device_fwd_bwd(flux, value, grad=grad, coef=1.0, shifts=None)
    torch.cuda.synchronize()
    assert np.isfinite(float(value)) and torch.isfinite(grad).all() and float(grad.abs().max()) > 0

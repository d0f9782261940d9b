"""CPU: the numpy restatement of a Lloyd step (tests/kmeans_cases.py) against a brute-force argmin of |x - c|^2, the
conditions its cases are chosen to meet, the host seeding `kmeans_plusplus`, the argument validation of `kmeans` and of
`GaussianMixtureModel.fit(init_params=...)` up to the point where a device is needed, and the C ABI of csrc/kmeans.hip
(declared, bound, built, and refusing bad arguments before it touches a device)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import kmeans_cases as cases

REPO = Path(__file__).resolve().parent.parent
ALL_CASES = [(*c, "separated") for c in cases.STEP_CASES] + [(*c, "overlap") for c in cases.OVERLAP_CASES]
NEW_SYMBOLS = ("jd_kmeans_create", "jd_kmeans_destroy", "jd_kmeans_step", "jd_gmm_fit_step_labels")


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: cases.case_name(*c))
def test_restatement_equals_brute_force(case):
    x, centres = cases.case_inputs(*case)
    ref = cases.reference(*case)
    x64, c64 = x.astype(np.float64), centres.astype(np.float64)
    dist = ((x64[:, None, :] - c64[None, :, :]) ** 2).sum(axis=2)
    brute = dist.argmin(axis=1)
    decided = ~ref["ambiguous"]
    assert np.array_equal(ref["float64"]["labels"][decided], brute[decided])
    assert ref["float64"]["unassigned"] == 0 and ref["float64"]["counts"].sum() == x.shape[0]
    picked = dist[np.arange(x.shape[0]), ref["float64"]["labels"]]
    assert abs(ref["float64"]["inertia"] - picked.sum()) <= 1e-10 * picked.sum()
    counts, sums = ref["float64"]["counts"], ref["float64"]["sums"]
    for k in range(case[1]):
        assert counts[k] == (ref["float64"]["labels"] == k).sum()
        assert np.allclose(sums[k], x64[ref["float64"]["labels"] == k].sum(axis=0), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: cases.case_name(*c))
def test_cases_meet_their_conditions_in_float32(case):
    """What the GPU tests ask of the device holds for the float32 restatement: outside the ambiguous set its labels are
    the float64 ones; the set is empty for separated clusters and at most 1 % for the overlapping ones."""
    ref = cases.reference(*case)
    ambiguous = ref["ambiguous"]
    if case[3] == "separated":
        assert not ambiguous.any()
    else:
        assert ambiguous.mean() <= cases.AMBIGUOUS_MAX
        assert np.isfinite(ref["float64"]["margin"]).all() and ref["float64"]["margin"].min() < 1.0  # the clusters do overlap
    assert np.array_equal(ref["float32"]["labels"][~ambiguous], ref["float64"]["labels"][~ambiguous])


def test_restatement_ties_nan_and_changed():
    x = np.zeros((4, 64), dtype=np.float32)
    x[1, 0] = 1.0
    x[2, 3] = np.nan
    centres = np.zeros((3, 64), dtype=np.float32)
    centres[2, 0] = 1.0  # centres 0 and 1 are identical
    step = cases.lloyd_step(x, centres, np.float64, old_labels=np.array([0, 0, 0, 1], dtype=np.int32))
    assert step["labels"].tolist() == [0, 2, -1, 0] and step["unassigned"] == 1 and step["changed"] == 3
    assert step["counts"].tolist() == [2, 0, 1] and np.isfinite(step["sums"]).all() and step["inertia"] == 0.0
    assert np.array_equal(step["centres"][1], centres[1])  # an empty cluster keeps its centre


def test_kmeans_plusplus_rows_are_distinct_and_deterministic():
    from jolideco_amd.priors.patches import kmeans_plusplus

    rs = np.random.RandomState(3)
    sample = rs.standard_normal((400, 64)).astype(np.float32)
    sample[200:] = sample[:200]  # every row twice
    a = kmeans_plusplus(sample, 50, 11)
    b = kmeans_plusplus(sample, 50, np.random.RandomState(11))
    c = kmeans_plusplus(sample, 50, 12)
    assert a.shape == (50, 64) and a.dtype == np.float64 and np.array_equal(a, b) and not np.array_equal(a, c)
    assert len({row.tobytes() for row in a}) == 50
    rows = {row.tobytes() for row in sample.astype(np.float64)}
    assert all(row.tobytes() in rows for row in a)
    assert len({row.tobytes() for row in kmeans_plusplus(sample, 200, 0)}) == 200  # every distinct row
    with pytest.raises(ValueError, match="distinct patches"):
        kmeans_plusplus(sample, 201, 0)
    with pytest.raises(ValueError, match="fewer than the 5"):
        kmeans_plusplus(sample[:4], 5, 0)
    with pytest.raises(ValueError, match="non-finite"):
        kmeans_plusplus(np.full((4, 64), np.nan), 2, 0)


@pytest.mark.parametrize("seed", range(5))
def test_kmeans_plusplus_takes_one_seed_per_blob(seed):
    from jolideco_amd.priors.patches import kmeans_plusplus

    rs = np.random.RandomState(100 + seed)
    blobs = rs.standard_normal((12, 64)) * 10.0
    label = np.repeat(np.arange(12), 40)
    sample = blobs[label] + 0.1 * rs.standard_normal((label.size, 64))
    seeds = kmeans_plusplus(sample, 12, seed)
    nearest = ((seeds[:, None, :] - blobs[None]) ** 2).sum(axis=2).argmin(axis=1)
    assert sorted(nearest.tolist()) == list(range(12))


def test_kmeans_validates_its_arguments():
    from jolideco_amd.priors.patches import kmeans

    x = torch.zeros(100, 64)
    with pytest.raises(ValueError, match=r"shape \(n, D\)"):
        kmeans(torch.zeros(100), 3)
    with pytest.raises(ValueError, match=r"shape \(n, D\)"):
        kmeans(torch.zeros(100, 64, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="D = 64 or D = 256"):
        kmeans(torch.zeros(100, 100), 3)
    with pytest.raises(ValueError, match="1024"):
        kmeans(torch.zeros(2000, 64), 1025)
    with pytest.raises(ValueError, match="1024"):
        kmeans(x, 0)
    with pytest.raises(ValueError, match="distinct patches"):
        kmeans(x, 101)
    with pytest.raises(ValueError, match="max_iter"):
        kmeans(x, 3, max_iter=0)
    with pytest.raises(ValueError, match="does not fit"):
        kmeans(x, 3, centres_init=np.zeros((3, 63)))
    with pytest.raises(ValueError, match="non-finite"):
        kmeans(x, 3, centres_init=np.full((3, 64), np.inf))
    with pytest.raises(ValueError, match="n_seed"):
        kmeans(x, 3, n_seed=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        kmeans(x, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        kmeans(x, 3, centres_init=np.zeros((3, 64)))


def test_fit_validates_init_params():
    from jolideco_amd.priors.patches import GaussianMixtureModel

    fit = GaussianMixtureModel.fit
    x = torch.zeros(100, 64)
    means, covs, weights = np.zeros((3, 64)), np.tile(np.eye(64), (3, 1, 1)), np.full(3, 1 / 3)
    model = GaussianMixtureModel.from_numpy(means, covs, weights)
    with pytest.raises(ValueError, match="init_params"):
        fit(x, 3, init_params="k-means++")
    for name in ("kmeans", "random-patches"):
        with pytest.raises(ValueError, match="cannot be given with"):
            fit(x, init=model, init_params=name)
        with pytest.raises(ValueError, match="cannot be given with"):
            fit(x, means_init=means, covariances_init=covs, weights_init=weights, init_params=name)
        with pytest.raises(ValueError, match="n_components is needed"):
            fit(x, init_params=name)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fit(x, 3, init_params=name)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianMixtureModel.fit_images(torch.zeros(32, 32), n_components=2, init_params="kmeans")


def test_new_symbols_are_declared_bound_and_built():
    from jolideco_amd import _hip, ops

    header = (REPO / "include" / "jolideco_hip.h").read_text()
    lib = _hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header) and name in _hip.EXPORTS and hasattr(lib, name)
    assert "kmeans.hip" in (REPO / "jolideco_amd" / "csrc" / "Makefile").read_text()
    assert hasattr(ops, "KMeansHandle") and "KMeansHandle" in ops.__all__


def test_c_abi_refuses_bad_arguments():
    """Null handles and pointers, D = 100, K = 0 and 1025, n = 0 and n past (2^31 - 1) / D return JD_ERR_INVALID (-1) with a
    message; the pointers are never dereferenced and nothing reaches a device."""
    from jolideco_amd import _hip

    lib = _hip.lib()
    handle = ctypes.c_void_p()
    assert lib.jd_kmeans_create(100, 4, 0, ctypes.byref(handle)) == -1 and not handle.value
    assert b"D = 64 or D = 256" in lib.jd_last_error() and b"100" in lib.jd_last_error()
    assert lib.jd_kmeans_create(64, 0, 0, ctypes.byref(handle)) == -1 and not handle.value
    assert b"1 <= K <= 1024" in lib.jd_last_error() and b"K = 0" in lib.jd_last_error()
    assert lib.jd_kmeans_create(256, 1025, 0, ctypes.byref(handle)) == -1 and b"K = 1025" in lib.jd_last_error()
    assert lib.jd_kmeans_create(64, 4, -1, ctypes.byref(handle)) == -1 and b"max_blocks" in lib.jd_last_error()
    assert lib.jd_kmeans_create(64, 4, 0, None) == -1 and b"null argument" in lib.jd_last_error()
    dummy = ctypes.c_void_p(64)
    assert lib.jd_kmeans_step(None, dummy, 16, dummy, dummy, dummy, None) == -1 and b"null handle" in lib.jd_last_error()
    assert lib.jd_kmeans_destroy(None) == 0
    assert lib.jd_gmm_fit_step_labels(None, dummy, 16, dummy, dummy, dummy, None) == -1 and b"null handle" in lib.jd_last_error()
    # creating a handle allocates nothing on a device and launches nothing (it only asks the runtime for the number of
    # compute units, and assumes 256 where there is no device); the pointers below are never dereferenced
    assert lib.jd_kmeans_create(256, 200, 0, ctypes.byref(handle)) == 0 and handle.value
    try:
        for args in ((None, 16, dummy, dummy, dummy), (dummy, 16, None, dummy, dummy), (dummy, 16, dummy, None, dummy),
                     (dummy, 16, dummy, dummy, None)):
            assert lib.jd_kmeans_step(handle, *args, None) == -1 and b"null argument" in lib.jd_last_error()
        assert lib.jd_kmeans_step(handle, dummy, 0, dummy, dummy, dummy, None) == -1 and b"n = 0" in lib.jd_last_error()
        too_many = (2**31 - 1) // 256 + 1
        assert lib.jd_kmeans_step(handle, dummy, too_many, dummy, dummy, dummy, None) == -1
        assert str(too_many).encode() in lib.jd_last_error()
        assert lib.jd_kmeans_step(handle, ctypes.c_void_p(66), 16, dummy, dummy, dummy, None) == -1
        assert b"aligned" in lib.jd_last_error()
    finally:
        assert lib.jd_kmeans_destroy(handle) == 0
    fit = ctypes.c_void_p()
    assert lib.jd_gmm_fit_create(64, 4, 0, ctypes.byref(fit)) == 0
    try:
        assert lib.jd_gmm_fit_step_labels(fit, dummy, 16, dummy, None, dummy, None) == -1 and b"null argument" in lib.jd_last_error()
        assert lib.jd_gmm_fit_step_labels(fit, dummy, 0, dummy, dummy, dummy, None) == -1 and b"n = 0" in lib.jd_last_error()
    finally:
        assert lib.jd_gmm_fit_destroy(fit) == 0


def test_the_five_step_run_is_decided_at_every_step():
    x, init = cases.five_inputs()
    steps = cases.five_reference()
    assert [s["changed"] for s in steps] == [1500, 283, 66, 1, 0]
    centres = [np.asarray(init, dtype=np.float64)] + [s["centres"] for s in steps]
    for step, c in zip(steps, centres):
        assert (step["margin"] > cases.tau(x, c)).all()

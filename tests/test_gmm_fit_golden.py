"""CPU: the float64 restatement of an EM step (tests/gmm_fit_cases.py) reproduces the scikit-learn fixture
tests/golden/gmm_fit.npz (tools/make_golden_gmm_fit.py) and, where it is installed, live scikit-learn; the C ABI of the
fit refuses bad arguments with a message before it touches a device; `GaussianMixtureModel.fit` validates its arguments."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import gmm_fit_cases as cases

RUNS = [(case, 1, cases.REG_COVAR, cases.case_name(*case)) for case in cases.STEP_CASES]
RUNS += [(cases.FIVE_CASE, cases.FIVE_STEPS, reg, f"five_reg{reg:g}") for reg in cases.FIVE_REGS]


def rel(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max()


@pytest.mark.parametrize("case, steps, reg, name", RUNS, ids=[r[3] for r in RUNS])
def test_restatement_reproduces_the_fixture(golden, case, steps, reg, name):
    fixture = golden("gmm_fit")
    x, weights, means, covariances = cases.case_inputs(*case)
    assert np.array_equal(fixture[f"{name}/weights_init"], weights) and np.array_equal(fixture[f"{name}/means_init"], means)
    got = cases.reference(*case, steps, reg)["float64"]
    assert rel(got[0], fixture[f"{name}/weights"]) < 1e-8
    assert rel(got[1], fixture[f"{name}/means"]) < 1e-8
    assert rel(cases.cov_sample(got[2]), fixture[f"{name}/covariances_sample"]) < 1e-8
    assert fixture[f"{name}/lower_bounds"].shape == (steps,) and rel(got[3], fixture[f"{name}/lower_bounds"]) < 1e-8
    assert str(fixture[f"{name}/source"]) == ("restatement" if case[2] < 2 else "sklearn")


@pytest.mark.parametrize("case", [c for c in cases.STEP_CASES if c[2] >= 2], ids=lambda c: cases.case_name(*c))
def test_restatement_reproduces_live_scikit_learn(case):
    mixture = pytest.importorskip("sklearn.mixture")
    x, weights, means, covariances = cases.case_inputs(*case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ConvergenceWarning: one step on purpose
        gm = mixture.GaussianMixture(n_components=case[1], covariance_type="full", tol=0.0, reg_covar=cases.REG_COVAR, max_iter=1,
                                     weights_init=weights, means_init=means, precisions_init=np.linalg.inv(covariances))
        gm.fit(x.astype(np.float64))
    got = cases.reference(*case)["float64"]
    assert rel(got[0], gm.weights_) < 1e-8 and rel(got[1], gm.means_) < 1e-8 and rel(got[2], gm.covariances_) < 1e-8
    assert rel(got[3], [gm.lower_bound_]) < 1e-8


def test_host_finish_equals_the_restatement():
    """`em_m_step` on exact float64 moments about the start means is the restatement's M-step: the algebra of the
    mean correction, without a device."""
    from jolideco_amd.priors.patches.gmm import em_m_step

    x, weights, means, covariances = cases.case_inputs(64, 5, 1000)
    x = x.astype(np.float64)
    l = cases.log_prob(x, weights, means, covariances)
    resp = np.exp(l - np.logaddexp.reduce(l, axis=1)[:, None])
    d = x[:, None, :] - means[None]
    s0, s1 = resp.sum(axis=0), np.einsum("nk,nkd->kd", resp, d)
    s2 = np.einsum("nk,nkd,nke->kde", resp, d, d)
    got = em_m_step(means, s0, s1, s2, x.shape[0], cases.REG_COVAR)
    ref = cases.reference(64, 5, 1000)["float64"]
    assert rel(got[0], ref[1]) < 1e-12 and rel(got[1], ref[2]) < 1e-11 and rel(got[2], ref[0]) < 1e-12


def test_c_abi_refuses_bad_arguments():
    """Null handles, D = 100, K = 0 and K = 1025 return JD_ERR_INVALID (-1) with a message; nothing reaches a device."""
    from jolideco_amd import _hip

    lib = _hip.lib()
    handle = ctypes.c_void_p()
    assert lib.jd_gmm_fit_create(100, 4, 0, ctypes.byref(handle)) == -1 and not handle.value
    assert b"D = 64 or D = 256" in lib.jd_last_error() and b"100" in lib.jd_last_error()
    assert lib.jd_gmm_fit_create(64, 0, 0, ctypes.byref(handle)) == -1 and not handle.value
    assert b"1 <= K <= 1024" in lib.jd_last_error() and b"K = 0" in lib.jd_last_error()
    assert lib.jd_gmm_fit_create(256, 1025, 0, ctypes.byref(handle)) == -1 and not handle.value
    assert b"K = 1025" in lib.jd_last_error()
    assert lib.jd_gmm_fit_create(64, 4, -1, ctypes.byref(handle)) == -1 and b"max_blocks" in lib.jd_last_error()
    assert lib.jd_gmm_fit_create(64, 4, 0, None) == -1 and b"null argument" in lib.jd_last_error()
    dummy = ctypes.c_void_p(64)
    assert lib.jd_gmm_fit_step(None, dummy, 16, dummy, dummy, dummy, dummy, None) == -1
    assert b"null handle" in lib.jd_last_error()
    assert lib.jd_gmm_fit_destroy(None) == 0


def test_fit_validates_its_arguments():
    from jolideco_amd.priors.patches import GaussianMixtureModel

    fit = GaussianMixtureModel.fit
    x = torch.zeros(100, 64)
    means, covs, weights = np.zeros((3, 64)), np.tile(np.eye(64), (3, 1, 1)), np.full(3, 1 / 3)
    start = dict(means_init=means, covariances_init=covs, weights_init=weights)
    model = GaussianMixtureModel.from_numpy(means, covs, weights)
    with pytest.raises(ValueError, match="not both"):
        fit(x, init=model, means_init=means)
    with pytest.raises(ValueError, match="together"):
        fit(x, means_init=means, weights_init=weights)
    with pytest.raises(ValueError, match="does not fit"):
        fit(x, **{**start, "covariances_init": covs[:2]})
    with pytest.raises(ValueError, match="does not fit"):
        fit(x, **{**start, "means_init": np.zeros((3, 63))})
    with pytest.raises(ValueError, match="n_components = 4"):
        fit(x, 4, **start)
    with pytest.raises(ValueError, match=r"shape \(n, D\)"):
        fit(torch.zeros(100), 3)
    with pytest.raises(ValueError, match=r"shape \(n, D\)"):
        fit(torch.zeros(100, 64, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="D = 64 or D = 256"):
        fit(torch.zeros(100, 100), 3)
    with pytest.raises(ValueError, match="n_components is needed"):
        fit(x)
    with pytest.raises(ValueError, match="1024"):
        fit(torch.zeros(2000, 64), 1025)
    with pytest.raises(ValueError, match="distinct patches"):
        fit(x, 101)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(x, **start)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(x, init=model)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianMixtureModel.fit_images(torch.zeros(32, 32), n_components=2)
    with pytest.raises(ValueError, match="sets `meta` itself"):
        GaussianMixtureModel.fit_images(torch.zeros(32, 32), n_components=2, meta=None)

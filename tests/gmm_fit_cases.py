"""Shared by tools/make_golden_gmm_fit.py, tests/test_gmm_fit_golden.py (CPU) and tests/test_gpu_gmm_fit.py (GPU): the
cases of the EM fit of a full-covariance Gaussian mixture, and `em_step`, a restatement of one step of
``sklearn.mixture.GaussianMixture(covariance_type="full")`` in numpy.  In float64 it is the reference of the GPU tests
(pinned against scikit-learn by tests/golden/gmm_fit.npz); run in float32 its distance from the float64 run is e_ref, the
error of an equally rounded evaluation, which sets the GPU tests' bounds.

Inputs are regenerated from seeds (`case_inputs`): the fixture stores the start's weights and means as a guard against a
drifting generator, and the results."""
import functools

import numpy as np
from scipy.linalg import solve_triangular

REG_COVAR = 1e-6
# (D, K, n): one patch; one short of and one past a 32-patch tile; a K that fills no tile; ragged last blocks; D = 256
STEP_CASES = [(64, 1, 1), (64, 3, 31), (64, 3, 33), (64, 5, 1000), (64, 17, 4099), (256, 2, 600)]
FIVE_CASE = (64, 3, 4099)
FIVE_STEPS = 5
# ridges of the five-step case: the default, under which the mean-free patches leave the covariances a direction that only
# the ridge holds up (condition 4e6: a float32 Cholesky factor, and with it e_ref of the lower bound, is poor), and a
# large one, under which e_ref is that of well-conditioned arithmetic
FIVE_REGS = (1e-6, 1e-2)
COV_SAMPLES = 8192  # covariance entries of a case the fixture keeps (all of them where there are no more)


def case_name(D, K, n):
    return f"d{D}_k{K}_n{n}"


def mean_free_patches(rs, D, n, n_clusters=4):
    """(n, D) float32 patches drawn from a few anisotropic clusters, each patch minus its own mean (what the
    subtract-mean patch norm hands the mixture)."""
    centres = rs.standard_normal((n_clusters, D)) * 2.0
    mixing = rs.standard_normal((n_clusters, D, D)) / np.sqrt(D) * np.linspace(0.3, 1.5, D)[None, None, :]
    label = rs.randint(0, n_clusters, size=n)
    z = rs.standard_normal((n, D))
    x = centres[label] + np.einsum("nd,nde->ne", z, mixing[label])
    x -= x.mean(axis=1, keepdims=True)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_inputs(D, K, n):
    """(x float32 (n, D), weights, means, covariances float64) of a case: data and a well-conditioned start.  The start
    means are K of the patches plus a small offset (distinct patches as far as n allows), the start covariances random
    symmetric positive definite matrices of the data's scale -- not the data covariance, which is singular for n < D."""
    rs = np.random.RandomState(1000 * D + 10 * K + n % 7)
    x = mean_free_patches(rs, D, n)
    pick = rs.choice(n, K, replace=n < K)
    means = x[pick].astype(np.float64) + 0.05 * rs.standard_normal((K, D))
    a = rs.standard_normal((K, D, D)) / np.sqrt(D)
    covariances = 0.6 * np.einsum("kij,klj->kil", a, a) + 0.4 * np.eye(D)[None]
    weights = rs.uniform(0.5, 1.5, size=K)
    weights /= weights.sum()
    for arr in (x, weights, means, covariances):
        arr.setflags(write=False)
    return x, weights, means, covariances


def precision_cholesky(covariances):
    """P_k = (L_k^-1)^T with cov_k = L_k L_k^T, in the dtype of the argument"""
    out = np.empty_like(covariances)
    eye = np.eye(covariances.shape[1], dtype=covariances.dtype)
    for k, cov in enumerate(covariances):
        out[k] = solve_triangular(np.linalg.cholesky(cov), eye, lower=True).T
    return out


def log_prob(x, weights, means, covariances):
    """(n, K) l_nk = log w_k + log N(x_n | mu_k, Sigma_k) in the dtype of `x`"""
    dtype = x.dtype
    D = x.shape[1]
    prec = precision_cholesky(covariances.astype(dtype))
    log_det = np.log(np.diagonal(prec, axis1=1, axis2=2)).sum(axis=1)
    out = np.empty((x.shape[0], weights.shape[0]), dtype=dtype)
    for k in range(weights.shape[0]):
        y = (x - means[k].astype(dtype)) @ prec[k]
        out[:, k] = dtype.type(-0.5) * (dtype.type(D * np.log(2 * np.pi)) + np.sum(y * y, axis=1)) + log_det[k]
    return out + np.log(weights.astype(dtype))


def em_step(x, weights, means, covariances, reg_covar=REG_COVAR, dtype=np.float64):
    """One EM step with every operation in `dtype`: (weights', means', covariances', lower bound, N)."""
    dtype = np.dtype(dtype)
    x = np.asarray(x).astype(dtype)
    n, D = x.shape
    l = log_prob(x, np.asarray(weights), np.asarray(means), np.asarray(covariances))
    top = l.max(axis=1, keepdims=True)
    lse = top[:, 0] + np.log(np.exp(l - top).sum(axis=1))
    resp = np.exp(l - lse[:, None])
    N = resp.sum(axis=0) + dtype.type(10 * np.finfo(np.float64).eps)
    new_means = (resp.T @ x) / N[:, None]
    new_cov = np.empty((N.shape[0], D, D), dtype=dtype)
    for k in range(N.shape[0]):
        diff = x - new_means[k]
        new_cov[k] = (resp[:, k, None] * diff).T @ diff / N[k]
        new_cov[k].flat[:: D + 1] += dtype.type(reg_covar)
    new_weights = N / dtype.type(n)
    new_weights = new_weights / new_weights.sum()
    return new_weights, new_means, new_cov, lse.mean(), N


def em_steps(x, weights, means, covariances, steps, reg_covar=REG_COVAR, dtype=np.float64):
    """`steps` EM steps: the final (weights, means, covariances) and the lower bound of every step"""
    bounds = []
    for _ in range(steps):
        weights, means, covariances, bound, _ = em_step(x, weights, means, covariances, reg_covar, dtype)
        bounds.append(float(bound))
    return weights, means, covariances, np.array(bounds)


@functools.lru_cache(maxsize=None)
def reference(D, K, n, steps=1, reg_covar=REG_COVAR):
    """float64 and float32 runs of a case (computed once, shared by the tests that need them, never modified)"""
    x, weights, means, covariances = case_inputs(D, K, n)
    return {dtype: em_steps(x, weights, means, covariances, steps, reg_covar, dtype) for dtype in ("float64", "float32")}


def cov_sample(covariances):
    """The covariance entries the fixture keeps: all, or every step-th of the flattened array (step odd, so the
    sample walks through all rows, columns and components)"""
    flat = np.asarray(covariances).reshape(-1)
    step = -(-flat.size // COV_SAMPLES)
    step += 1 - step % 2
    return flat[::step]


# ---- error measures of the GPU tests ---------------------------------------------------------------------------------
def rel_max(got, ref, scale=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() if scale is None else scale))


def errors(got, ref, start_means):
    """Errors of a result (weights, means, covariances, bounds) against the float64 `ref`, one per quantity, each relative
    to the largest entry of the quantity.  The covariances are measured against the second moments about the START means,
    max |Sigma'_k + delta_k delta_k^T| with delta = mu' - mu: the device accumulates the moments about the means it was
    given, so that -- not Sigma' alone, which is reg_covar for a single patch -- is the size of what float32 rounds."""
    delta = np.asarray(ref[1], dtype=np.float64) - np.asarray(start_means, dtype=np.float64)
    moment = np.asarray(ref[2], dtype=np.float64) + delta[:, :, None] * delta[:, None, :]
    return {
        "weights": rel_max(got[0], ref[0]),
        "means": rel_max(got[1], ref[1]),
        "covariances": rel_max(got[2], ref[2], scale=np.abs(moment).max()),
        "lower_bound": rel_max(got[3], ref[3]),
    }

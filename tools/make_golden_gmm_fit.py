"""Generate tests/golden/gmm_fit.npz with scikit-learn on the CPU.

Run:  python tools/make_golden_gmm_fit.py

For every case of tests/gmm_fit_cases.py (`STEP_CASES`: one EM step; `FIVE_CASE` with each ridge of `FIVE_REGS`: five
steps) ``sklearn.mixture.GaussianMixture(covariance_type="full", tol=0, max_iter=steps)`` is run from the case's start
(`weights_init`, `means_init`, `precisions_init` = the inverse start covariances) and its weights, means, covariances and
lower bound are stored -- the five-step cases with the lower bound after every step (runs with max_iter = 1 .. 5).
The inputs are regenerated from seeds by `gmm_fit_cases.case_inputs`; the fixture holds the start's weights and means
only as a guard against a drifting generator.  Of a case's covariances it holds `gmm_fit_cases.cov_sample`: all entries
where there are at most 8192, else every step-th, which keeps the file at a few hundred kilobytes.
scikit-learn refuses a single sample; the one-patch case stores the float64 restatement instead (`source` says which).
While generating, the restatement `gmm_fit_cases.em_step` is asserted to reproduce scikit-learn to 1e-9.
"""
import sys
import warnings
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))

import gmm_fit_cases as cases  # noqa: E402


def sklearn_steps(x, weights, means, covariances, steps, reg_covar):
    from sklearn.mixture import GaussianMixture

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ConvergenceWarning: the runs stop at max_iter on purpose
        gm = GaussianMixture(n_components=len(weights), covariance_type="full", tol=0.0, reg_covar=reg_covar, max_iter=steps,
                             weights_init=weights, means_init=means, precisions_init=np.linalg.inv(covariances))
        gm.fit(x.astype(np.float64))
    return gm.weights_, gm.means_, gm.covariances_, gm.lower_bound_


def agree(got, ref, what):
    err = np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max()
    assert err < 1e-9, f"{what}: the restatement is {err:.2e} from scikit-learn"
    return err


def main():
    import sklearn

    out = {"sklearn_version": np.array(sklearn.__version__)}
    runs = [(case, 1, cases.REG_COVAR, cases.case_name(*case)) for case in cases.STEP_CASES]
    runs += [(cases.FIVE_CASE, cases.FIVE_STEPS, reg, f"five_reg{reg:g}") for reg in cases.FIVE_REGS]
    for case, steps, reg, name in runs:
        x, weights, means, covariances = cases.case_inputs(*case)
        mine = cases.em_steps(x, weights, means, covariances, steps, reg)
        if x.shape[0] < 2:
            result, bounds, source = mine[:3], mine[3], "restatement"
        else:
            source = "sklearn"
            bounds = np.array([sklearn_steps(x, weights, means, covariances, i, reg)[3] for i in range(1, steps + 1)])
            result = sklearn_steps(x, weights, means, covariances, steps, reg)[:3]
            worst = max(agree(mine[i], result[i], f"{name} {what}") for i, what in enumerate(("weights", "means", "covariances")))
            worst = max(worst, agree(mine[3], bounds, f"{name} lower bound"))
            print(f"{name}: restatement within {worst:.1e} of scikit-learn {sklearn.__version__}")
        out[f"{name}/source"] = np.array(source)
        out[f"{name}/weights_init"], out[f"{name}/means_init"] = weights, means
        out[f"{name}/weights"], out[f"{name}/means"] = result[0], result[1]
        out[f"{name}/covariances_sample"] = cases.cov_sample(result[2])
        out[f"{name}/lower_bounds"] = np.asarray(bounds, dtype=np.float64)
    path = REPO / "tests" / "golden" / "gmm_fit.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()

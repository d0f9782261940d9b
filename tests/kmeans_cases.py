"""Shared by tests/test_kmeans_host.py (CPU) and tests/test_gpu_kmeans.py (GPU): the cases of the k-means start of the
mixture fit and `lloyd_step`, a numpy restatement of one Lloyd step of csrc/kmeans.hip.  In float64 it is the reference of
the GPU tests; run in float32 its distance from the float64 run is e_ref, the error of an equally rounded evaluation.

Inputs are regenerated from seeds (`case_inputs`), as in gmm_fit_cases.py.

Labels are compared only where they are decided: two float32 evaluations of the scores s_nk = |c_k|^2 - 2 x_n . c_k in any
summation order differ by at most gamma_D (|x_n| |c_k| for the dot product, doubled) + gamma_D |c_k|^2 + one rounding of the
result, gamma_D = D 2^-24 / (1 - D 2^-24), i.e. by less than 4 D 2^-24 (|x_n| C + C^2) with C = max_k |c_k|; `tau` is twice
that, the bound on the difference of two such scores, and a patch whose float64 margin between its two smallest scores is
at most tau_n is `ambiguous`."""
import functools

import numpy as np

# (D, K, n): one patch; one short of and one past a 32-patch tile; a K that fills no 16-tile with a ragged last block; more
# than two centre tiles; D = 256; D = 256 at the reference's K
STEP_CASES = [(64, 1, 1), (64, 3, 31), (64, 3, 33), (64, 17, 4099), (64, 33, 1000), (256, 2, 600), (256, 200, 700)]
# one case of overlapping clusters per D: mean-free patches of a few broad clusters, the centres K of the patches (at D = 256
# K = 33 and not 200: with 200 of 700 patches as centres, near ties among the centres alone pass 1 % of the patches)
OVERLAP_CASES = [(64, 17, 4099), (256, 33, 700)]
AMBIGUOUS_MAX = 0.01  # share of ambiguous patches an overlapping case may have
FIVE_CASE = (64, 5, 1500)
FIVE_STEPS = 5


def case_name(D, K, n, kind="separated"):
    return f"d{D}_k{K}_n{n}_{kind}"


@functools.lru_cache(maxsize=None)
def case_inputs(D, K, n, kind="separated"):
    """(x float32 (n, D), centres float32 (K, D)), read-only.  "separated": K tight blobs far apart, the centres the blob
    centres a little displaced, so every margin is large.  "overlap": broad overlapping clusters, the centres K of the
    patches (with replacement only where n < K)."""
    rs = np.random.RandomState(7000 * D + 10 * K + n % 11 + (kind == "overlap"))
    if kind == "separated":
        blobs = rs.standard_normal((K, D)) * 3.0
        label = rs.randint(0, K, size=n)
        x = (blobs[label] + 0.5 * rs.standard_normal((n, D))).astype(np.float32)
        centres = (blobs + 0.1 * rs.standard_normal((K, D))).astype(np.float32)
    else:
        n_clusters = 4
        means = rs.standard_normal((n_clusters, D)) * 2.0
        mixing = rs.standard_normal((n_clusters, D, D)) / np.sqrt(D) * np.linspace(0.3, 1.5, D)[None, None, :]
        label = rs.randint(0, n_clusters, size=n)
        x = means[label] + np.einsum("nd,nde->ne", rs.standard_normal((n, D)), mixing[label])
        x = (x - x.mean(axis=1, keepdims=True)).astype(np.float32)
        centres = x[rs.choice(n, K, replace=n < K)].copy()
    x.setflags(write=False)
    centres.setflags(write=False)
    return x, centres


def cluster_sums(x, labels, K):
    """float64 (count (K,), sum x (K, D)) of the patches with label k; labels outside [0, K) are in no sum"""
    x = np.asarray(x, dtype=np.float64)
    counts, sums = np.zeros(K), np.zeros((K, x.shape[1]))
    for k in range(K):
        member = labels == k
        counts[k] = member.sum()
        sums[k] = x[member].sum(axis=0)
    return counts, sums


def lloyd_step(x, centres, dtype=np.float64, old_labels=None):
    """One Lloyd step with the scores in `dtype` by the expanded formula, lowest-index ties, -1 for a patch with a
    non-finite score, float64 cluster sums, centres rounded to float32 (an empty cluster keeps its centre).  Returns a
    dict: labels, counts, sums, inertia, changed, unassigned, centres (float64 holding float32 values), margin (between
    the two smallest scores; inf for K = 1 and for unassigned patches)."""
    dtype = np.dtype(dtype)
    xd, cd = np.asarray(x).astype(dtype), np.asarray(centres).astype(dtype)
    K = cd.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        scores = (cd * cd).sum(axis=1)[None, :] - dtype.type(2) * (xd @ cd.T)
        good = np.isfinite(scores).all(axis=1)
        labels = np.where(good, np.argmin(np.where(np.isfinite(scores), scores, np.inf), axis=1), -1).astype(np.int32)
        picked = np.take_along_axis(scores, np.maximum(labels, 0)[:, None].astype(np.int64), axis=1)[:, 0]
        inertia = float(np.maximum((xd * xd).sum(axis=1) + picked, 0)[good].sum(dtype=dtype))
        if K > 1:
            two = np.partition(np.where(np.isfinite(scores), scores, np.inf), 1, axis=1)[:, :2]
            margin = np.where(good, two[:, 1] - two[:, 0], np.inf)
        else:
            margin = np.full(xd.shape[0], np.inf)
    counts, sums = cluster_sums(x, labels, K)
    new = np.asarray(centres, dtype=np.float64).copy()
    filled = counts > 0
    new[filled] = (sums[filled] / counts[filled, None]).astype(np.float32).astype(np.float64)
    changed = int(xd.shape[0]) if old_labels is None else int((labels != old_labels).sum())
    return {"labels": labels, "counts": counts, "sums": sums, "inertia": inertia, "changed": changed,
            "unassigned": int((~good).sum()), "centres": new, "margin": margin}


def tau(x, centres):
    """tau_n = 8 D 2^-24 (|x_n| C + C^2), C = max_k |c_k| (module docstring)"""
    x, centres = np.asarray(x, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    C = np.sqrt((centres * centres).sum(axis=1)).max()
    return 8.0 * x.shape[1] * 2.0**-24 * (np.sqrt((x * x).sum(axis=1)) * C + C * C)


@functools.lru_cache(maxsize=None)
def reference(D, K, n, kind="separated"):
    """float64 and float32 runs of a case and its ambiguous set (computed once, shared, never modified)"""
    x, centres = case_inputs(D, K, n, kind)
    out = {name: lloyd_step(x, centres, name) for name in ("float64", "float32")}
    out["ambiguous"] = ~(out["float64"]["margin"] > tau(x, centres))
    return out


def lloyd_steps(x, centres, steps):
    """`steps` float64 Lloyd steps from `centres`: the list of the step dicts (centres of step i: result[i]["centres"])"""
    out, labels = [], np.full(np.asarray(x).shape[0], -1, dtype=np.int32)
    centres = np.asarray(centres, dtype=np.float64)
    for _ in range(steps):
        step = lloyd_step(x, centres, np.float64, labels)
        out.append(step)
        if step["changed"] == 0:
            break
        labels, centres = step["labels"], step["centres"]
    return out


@functools.lru_cache(maxsize=None)
def five_inputs():
    """(x, centres_init) of the multi-iteration run: eight blobs for five centres started at five of the patches, so
    that labels keep changing for four steps (1500, 283, 66, 1, 0 changes) while every margin stays above tau"""
    D, K, n = FIVE_CASE
    rs = np.random.RandomState(500)
    blobs = rs.standard_normal((8, D))
    label = rs.randint(0, 8, size=n)
    x = (blobs[label] + 0.45 * rs.standard_normal((n, D))).astype(np.float32)
    init = x[rs.choice(n, K, replace=False)].copy()
    x.setflags(write=False)
    init.setflags(write=False)
    return x, init


@functools.lru_cache(maxsize=None)
def five_reference():
    x, init = five_inputs()
    return lloyd_steps(x, init, FIVE_STEPS)

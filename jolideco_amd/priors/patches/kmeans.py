"""k-means on image patches: the start of `GaussianMixtureModel.fit(init_params="kmeans")`.

Lloyd steps run on the GPU (csrc/kmeans.hip: assignment on v_mfma_f32_16x16x4_f32, cluster sums in float64, no atomics);
the seeding -- greedy k-means++ -- runs on the host in float64 on a subsample of the patches.  The scheme is
scikit-learn's (``KMeans(init="k-means++", n_init=1)``), not its random stream: the two agree statistically, not step by
step.  An empty cluster keeps its centre (scikit-learn relocates it)."""
from dataclasses import dataclass

import numpy as np
import torch

__all__ = ["kmeans", "kmeans_plusplus", "KMeansResult"]


@dataclass
class KMeansResult:
    """``centres`` float64 (K, D) holding float32 values, ``labels`` int32 device tensor (n,) (-1: a patch with a
    non-finite score), ``counts`` float64 (K,) of the last assignment, ``inertia`` one value per iteration, ``n_iter``,
    ``converged`` (an iteration changed no label), ``unassigned`` patches of the last assignment."""

    centres: np.ndarray
    labels: torch.Tensor
    counts: np.ndarray
    inertia: list
    n_iter: int
    converged: bool
    unassigned: int = 0


def kmeans_plusplus(sample, n_clusters, random_state):
    """Greedy k-means++ (Arthur & Vassilvitskii 2007, with scikit-learn's 2 + floor(ln K) local trials) on the rows of
    ``sample`` (m, D) in float64: the first centre is a uniform draw, every further one the best -- lowest potential -- of
    the trials drawn with probability proportional to the squared distance to the nearest centre chosen so far.
    ``random_state`` is a ``numpy.random.RandomState`` (drawn from in place) or a seed.  Returns (K, D) float64 rows of
    the sample, all distinct; ValueError when the sample holds fewer than K distinct rows.
    Cost: per seed one (trials, m) float64 distance matrix by a matrix product, 2 trials m D flops -- with the default
    m = 256 K of `kmeans` that is about 512 K^2 D (2 + ln K) flops in all: seconds at K = 200, D = 256, minutes (and a
    0.5 GB float64 sample) at K = 1024, D = 256, where a smaller ``n_seed`` is the remedy."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    x = np.ascontiguousarray(sample, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f"sample must be (m, D), got shape {x.shape}")
    m, K = x.shape[0], int(n_clusters)
    if K < 1:
        raise ValueError(f"n_clusters must be at least 1, got {K}")
    if m < K:
        raise ValueError(f"the sample holds {m} patches, fewer than the {K} distinct patches k-means++ needs")
    if not np.isfinite(x).all():
        raise ValueError("the sample holds non-finite values")
    trials = 2 + int(np.log(K))
    norms = np.einsum("md,md->m", x, x)

    def distances(rows):
        d = np.maximum(norms[rows][:, None] - 2.0 * (x[rows] @ x.T) + norms[None, :], 0.0)
        for i, r in enumerate(rows):  # a patch equal to a candidate is at distance 0, whatever the expansion rounds to
            d[i, r] = 0.0
            near = np.flatnonzero(d[i] <= 1e-9 * (norms[r] + 1e-300))
            d[i, near[(x[near] == x[r]).all(axis=1)]] = 0.0
        return d

    chosen = [int(rs.randint(m))]
    closest = distances(chosen)[0]
    for _ in range(1, K):
        potential = closest.sum()
        if not potential > 0.0:
            raise ValueError(f"the sample holds only {len(chosen)} distinct patches, fewer than the {K} k-means++ needs")
        candidates = np.searchsorted(np.cumsum(closest), rs.uniform(size=trials) * potential)
        candidates = np.minimum(candidates, m - 1)
        candidates = candidates[closest[candidates] > 0.0]  # (a draw on the edge of a zero-weight row)
        if candidates.size == 0:
            candidates = np.array([int(np.argmax(closest))])
        trial = np.minimum(closest[None, :], distances(list(candidates)))
        best = int(np.argmin(trial.sum(axis=1)))
        chosen.append(int(candidates[best]))
        closest = trial[best]
    return x[chosen].copy()


_KMEANS_HANDLES = {}


def _kmeans_handle(handle_cls, device, n_features, n_clusters):
    """The work space of (device, D, K), created on first use and kept (as `gmm._fit_handle` keeps the fit's)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), int(n_features), int(n_clusters))
    if key not in _KMEANS_HANDLES:
        _KMEANS_HANDLES[key] = handle_cls(n_features, n_clusters, device)
    return _KMEANS_HANDLES[key]


def _validate(patches, n_clusters, centres_init, max_iter):
    if not isinstance(patches, torch.Tensor) or patches.ndim != 2 or patches.dtype != torch.float32:
        raise ValueError("patches must be a float32 torch tensor of shape (n, D)")
    n, D = int(patches.shape[0]), int(patches.shape[1])
    if D not in (64, 256):
        raise ValueError(f"patches of D = 64 or D = 256 features only, got D = {D}")
    if n < 1 or n > (2**31 - 1) // D:
        raise ValueError(f"1 <= n <= (2^31 - 1) / D patches, got n = {n}")
    K = int(n_clusters)
    if not 1 <= K <= 1024:
        raise ValueError(f"1 <= n_clusters <= 1024, got {K}")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    if centres_init is not None:
        centres_init = np.array(centres_init, dtype=np.float64)
        if centres_init.shape != (K, D):
            raise ValueError(f"centres_init of shape {centres_init.shape} does not fit ({K}, {D})")
        if not np.isfinite(centres_init).all():
            raise ValueError("centres_init holds non-finite values")
    elif K > n:
        raise ValueError(f"{K} distinct patches as seeds need n >= {K}, got n = {n}")
    return n, D, K, centres_init


def kmeans(patches, n_clusters, *, centres_init=None, max_iter=100, random_state=0, n_seed=None):
    """Cluster ``patches`` (HIP float32 tensor (n, D), D = 64 or 256) into ``n_clusters`` clusters by Lloyd's algorithm.

    The start is ``centres_init`` (K, D) or, without it, `kmeans_plusplus` on ``n_seed`` patches (default
    min(n, max(256 K, 16384))) drawn without replacement by ``numpy.random.RandomState(random_state)``, which the seeding
    then continues to draw from.  Every iteration is one device step (assignment, cluster sums in float64) and the centre
    update on the host: c_k <- float32(sum x_k / count_k) with the division in float64; an empty cluster keeps its centre.
    The iteration stops when an assignment changes no label (``converged``) or after ``max_iter`` steps.  The labels and
    counts returned are those of the last assignment, i.e. of the centres BEFORE the last update when not converged.
    Returns a `KMeansResult`."""
    from ...ops import KMeansHandle
    from .gmm import _upload

    n, D, K, centres = _validate(patches, n_clusters, centres_init, max_iter)
    if n_seed is not None and not K <= int(n_seed):
        raise ValueError(f"n_seed = {n_seed} patches cannot seed {K} clusters")
    if not patches.is_cuda:
        raise RuntimeError("patches must be a HIP tensor: jolideco_amd has no CPU path")
    patches = patches.contiguous()
    device = patches.device
    if centres is None:
        rs = np.random.RandomState(random_state)
        m = min(n, max(256 * K, 16384)) if n_seed is None else min(n, int(n_seed))
        index = np.sort(rs.choice(n, m, replace=False))
        sample = patches[torch.from_numpy(index).to(device)].cpu().numpy()
        centres = kmeans_plusplus(sample, K, rs)
    centres = centres.astype(np.float32).astype(np.float64)

    handle = _kmeans_handle(KMeansHandle, device, D, K)
    labels = torch.full((n,), -1, dtype=torch.int32, device=device)
    inertia, converged, counts, unassigned = [], False, None, 0
    for _ in range(int(max_iter)):
        counts, sums, value, changed, unassigned = handle.step(patches, _upload(centres, device), labels)
        inertia.append(value)
        if changed == 0:
            converged = True
            break
        filled = counts > 0
        centres = centres.copy()
        centres[filled] = (sums[filled] / counts[filled, None]).astype(np.float32).astype(np.float64)
    return KMeansResult(centres=centres, labels=labels, counts=counts, inertia=inertia, n_iter=len(inertia), converged=converged,
                        unassigned=unassigned)

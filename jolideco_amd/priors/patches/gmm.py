"""Gaussian mixture model of image patches (reference: jolideco/priors/patches/gmm.py:64-299).

Constants are prepared on the host in float64/float32 exactly as the reference does (scipy
Cholesky -> precision Cholesky -> fp32), then handed to the HIP library which lays them out in
MFMA fragment order.  The trained GMM libraries of the reference ("zoran-weiss", ...) are external
data files that are not part of this repository: `from_registry` / `read` load them from
``$JOLIDECO_GMM_LIBRARY`` exactly as the reference does (gmm.py:301-391,493-508) when the user has them;
`from_numpy` takes explicit arrays; `fit` / `fit_images` train a mixture on the user's own patches (EM, csrc/gmm_fit.hip).
"""
import json
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from ...utils.norms import PatchNorm, SubtractMeanPatchNorm
from ...utils.numpy import compute_precision_cholesky, get_pixel_weights

__all__ = ["GaussianMixtureModel", "GaussianMixtureModelMeta", "GMMNotAvailableError"]


class GMMNotAvailableError(ValueError):
    """The named GMM is not in the user's GMM library (or there is no library)."""


@dataclass
class GaussianMixtureModelMeta:
    """Meta data: ``stride`` selects the overlap pixel weights, ``patch_norm`` the patch
    normalisation (jolideco/priors/patches/gmm.py:24-61)."""

    stride: Optional[int] = None
    patch_norm: PatchNorm = field(default_factory=SubtractMeanPatchNorm)

    @classmethod
    def from_table(cls, table):
        """Meta data of a GMM table file: patch norm from the ``PNPTYPE`` keyword, stride = half the
        patch edge (jolideco/priors/patches/gmm.py:38-61)."""
        patch_norm = PatchNorm.from_dict({"type": table.meta.get("PNPTYPE", "subtract-mean")})
        npix = int(table["means"].shape[-1] ** 0.5)
        return cls(stride=npix // 2, patch_norm=patch_norm)


def get_gmm_registry():
    """Index of the user's GMM library: ``$JOLIDECO_GMM_LIBRARY/jolideco-gmm-library-index.json``
    (jolideco/priors/patches/gmm.py:493-508; read on demand here, at import time there)."""
    path = Path(os.path.expandvars("$JOLIDECO_GMM_LIBRARY/jolideco-gmm-library-index.json"))
    if not path.exists():
        return {}
    with path.open() as f:
        return json.load(f)


def em_m_step(means, sum_r, sum_rd, sum_rdd, n, reg_covar):
    """Finish the M-step of EM in float64 from the weighted moments about the current ``means`` (K, D):
    ``sum_r`` (K,) = sum_n r_nk, ``sum_rd`` (K, D) = sum_n r_nk d, ``sum_rdd`` (K, D, D) = sum_n r_nk d d^T, d = x_n - means[k].
    With N_k = sum_r + 10 eps (scikit-learn's guard) and delta = sum_rd / N_k the new mean is means + delta, and the
    moments about it are sum_rdd - delta sum_rd^T - sum_rd delta^T + sum_r delta delta^T.  Returns (means, covariances,
    weights); the covariances are symmetrised and carry the ridge ``reg_covar``."""
    N = sum_r + 10 * np.finfo(np.float64).eps
    delta = sum_rd / N[:, None]
    new_means = means + delta
    outer = delta[:, :, None] * delta[:, None, :]
    cov = sum_rdd / N[:, None, None] - (2.0 - sum_r / N)[:, None, None] * outer
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    D = means.shape[1]
    cov[:, np.arange(D), np.arange(D)] += reg_covar
    weights = N / n
    return new_means, cov, weights / weights.sum()


def _upload(array, device):
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(device)


def em_step(handle, patches, means, covariances, weights, reg_covar):
    """One EM step of `GaussianMixtureModel.fit`: the float64 parameters go to the device as float32 means, precision
    factors (`compute_precision_cholesky`) and constants log w_k + log det P_k - D/2 log 2 pi (of the ROUNDED factors, so
    that the densities the device evaluates are normalised), ``handle`` (`ops.GmmFitHandle`) sums the responsibilities
    and the moments about those float32 means over ``patches``, and `em_m_step` finishes in float64.
    Returns (means, covariances, weights, lower bound, sum of the responsibilities per component)."""
    K, D = means.shape
    n = patches.shape[0]
    device = patches.device
    means32 = means.astype(np.float32)
    prec32 = np.empty((K, D, D), dtype=np.float32)
    for k in range(K):
        try:
            prec32[k] = compute_precision_cholesky(covariances[k : k + 1])[0]
        except ValueError as exc:
            raise ValueError(
                f"the covariance of component {k} is not positive definite (largest entry {np.abs(covariances[k]).max():.3g}, "
                f"reg_covar = {reg_covar:g}); raise reg_covar or rescale the patches"
            ) from exc
    diag = prec32.reshape(K, -1)[:, :: D + 1].astype(np.float64)
    const = np.log(weights) + np.log(diag).sum(axis=1) - 0.5 * D * np.log(2 * np.pi)
    s0, s1, s2, lse_sum = handle.step(patches, _upload(means32, device), _upload(prec32, device), _upload(const, device))
    new_means, new_cov, new_weights = em_m_step(means32.astype(np.float64), s0, s1, s2, n, reg_covar)
    return new_means, new_cov, new_weights, lse_sum / n, s0


def random_start(patches, n_components, reg_covar=1e-6, random_state=0):
    """The start `GaussianMixtureModel.fit` takes when it is given none: ``n_components`` distinct patches drawn by
    ``numpy.random.RandomState(random_state)`` as means, the covariance of all patches + ``reg_covar`` I for every
    component, uniform weights -- float64 (means, covariances, weights).  Mean and covariance of the patches come from the
    step kernel itself: one component with P = I and c = 0 has r = 1; a pass about zero gives the mean, a second one about
    that mean the moments."""
    from ...ops import GmmFitHandle

    n, D = patches.shape
    device = patches.device
    one = _fit_handle(GmmFitHandle, device, D, 1)
    eye, zero = _upload(np.eye(D)[None], device), _upload(np.zeros(1), device)
    _, s1, _, _ = one.step(patches, _upload(np.zeros((1, D)), device), eye, zero)
    centre = (s1 / n).astype(np.float32)
    s0, s1, s2 = one.step(patches, _upload(centre, device), eye, zero)[:3]
    _, cov_all, _ = em_m_step(centre.astype(np.float64), s0, s1, s2, n, reg_covar)
    index = np.sort(np.random.RandomState(random_state).choice(n, n_components, replace=False))
    means = patches[torch.from_numpy(index).to(device)].cpu().numpy().astype(np.float64)
    return means, np.repeat(cov_all, n_components, axis=0), np.full(n_components, 1.0 / n_components)


def kmeans_start(handle, patches, n_components, reg_covar=1e-6, random_state=0, max_iter=100, n_seed=None):
    """The start of `GaussianMixtureModel.fit(init_params="kmeans")`: `kmeans` clusters the patches, ``handle``
    (`ops.GmmFitHandle`) sums the moments of the hard assignments about the centres in one pass, and `em_m_step` turns
    them into float64 (means, covariances + ``reg_covar`` I, weights) -- scikit-learn's start from one-hot
    responsibilities.  The fourth result is the record `fit` keeps under ``fit_info["kmeans"]``."""
    from .kmeans import kmeans

    n, D = patches.shape
    result = kmeans(patches, n_components, max_iter=max_iter, random_state=random_state, n_seed=n_seed)
    if result.unassigned:
        raise ValueError(f"{result.unassigned} patches hold non-finite values: the k-means start cannot place them")
    starved = np.flatnonzero(~(result.counts >= D))
    if starved.size:
        raise ValueError(
            f"component {int(starved[0])} is starved by the k-means start: its cluster holds {int(result.counts[starved[0]])} patches, "
            f"fewer than the D = {D} patches a covariance needs (components {starved.tolist()}); choose fewer components or "
            "another random_state"
        )
    s0, s1, s2 = handle.step_labels(patches, _upload(result.centres, patches.device), result.labels)
    means, covariances, weights = em_m_step(result.centres, s0, s1, s2, n, reg_covar)
    info = {"inertia": list(result.inertia), "n_iter": result.n_iter, "converged": result.converged, "counts": result.counts,
            "means": means, "covariances": covariances, "weights": weights}
    return means, covariances, weights, info


_FIT_HANDLES = {}


def _fit_handle(handle_cls, device, n_features, n_components):
    """The fit work space of (device, D, K), created on first use and kept: later fits of the size allocate nothing."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), int(n_features), int(n_components))
    if key not in _FIT_HANDLES:
        _FIT_HANDLES[key] = handle_cls(n_features, n_components, device)
    return _FIT_HANDLES[key]


class GaussianMixtureModel:
    """Gaussian mixture model with full covariances.

    Parameters: fp32 numpy arrays ``means`` (K, D), ``covariances`` (K, D, D), ``weights`` (K,),
    ``precisions_cholesky`` (K, D, D).
    """

    def __init__(self, means, covariances, weights, precisions_cholesky, meta=None):
        self.means_numpy = np.asarray(means, dtype=np.float32)
        self.covariances_numpy = np.asarray(covariances, dtype=np.float32)
        self.weights_numpy = np.asarray(weights, dtype=np.float32)
        self.precisions_cholesky_numpy = np.asarray(precisions_cholesky, dtype=np.float32)
        self.meta = meta or GaussianMixtureModelMeta()
        self.registry_name = None
        self.fit_info = None  # set by `fit`
        self._handles = {}
        self._eigen_images = None  # (`eigen_images`, on first use)

    @classmethod
    def from_numpy(cls, means, covariances, weights, meta=None):
        """Create from float64 numpy arrays (jolideco/priors/patches/gmm.py:119-149)."""
        precisions_cholesky = compute_precision_cholesky(covariances=np.asarray(covariances))
        return cls(
            means=np.asarray(means).astype(np.float32),
            covariances=np.asarray(covariances).astype(np.float32),
            weights=np.asarray(weights).astype(np.float32),
            precisions_cholesky=precisions_cholesky.astype(np.float32),
            meta=meta,
        )

    @classmethod
    def from_sklearn_gmm(cls, gmm):
        return cls.from_numpy(means=gmm.means_, covariances=gmm.covariances_, weights=gmm.weights_)

    @classmethod
    def from_registry(cls, name, **kwargs):
        """Load a trained GMM by its name in the user's library index (gmm.py:301-335)."""
        registry = get_gmm_registry()
        if name not in registry:
            raise GMMNotAvailableError(
                f"Not a supported GMM {name}, choose from {list(registry)} (the index is "
                "$JOLIDECO_GMM_LIBRARY/jolideco-gmm-library-index.json; the library files are external data)"
            )
        kwargs.update(registry[name])
        gmm = cls.read(**kwargs)
        gmm.registry_name = name
        return gmm

    @classmethod
    def read(cls, filename, format="epll-matlab", **kwargs):
        """Read a trained GMM (gmm.py:336-391).

        format : {"epll-matlab", "epll-matlab-16x16", "table"}
            Zoran & Weiss EPLL ``.mat`` files (through scipy.io) or a FITS table with ``means`` (K, D),
            ``weights`` (K,) and ``covariances`` (K, D, D) columns.
        """
        filename = str(Path(os.path.expandvars(str(filename))))
        if format in ("epll-matlab", "epll-matlab-16x16"):
            import scipy.io as sio

            record = sio.loadmat(filename)["GS" if format == "epll-matlab" else "GMM"]
            covariances = record["covs"][0][0].T
            weights = record["mixweights"][0][0][:, 0]
            if format == "epll-matlab":
                means = record["means"][0][0].T
                meta = GaussianMixtureModelMeta(stride=4, patch_norm=SubtractMeanPatchNorm())
            else:
                means = np.zeros((200, 256))
                meta = GaussianMixtureModelMeta(stride=8, patch_norm=SubtractMeanPatchNorm())
        elif format == "table":
            from ...utils.io._fitsfile import read_fits

            tables = [hdu.data for hdu in read_fits(filename) if hdu.kind == "bintable"]
            if not tables:
                raise ValueError(f"{filename} holds no table")
            table = tables[0]
            means, weights, covariances = table["means"], table["weights"], table["covariances"]
            meta = GaussianMixtureModelMeta.from_table(table)
        else:
            raise ValueError(f"Not a supported format {format}")
        return cls.from_numpy(means=means, covariances=covariances, weights=weights, meta=meta, **kwargs)

    def write(self, filename, overwrite=False):
        """Write the model as a FITS table that `read(format="table")` -- of this package and of the
        reference -- loads back."""
        from ...utils.io._fitsfile import HDU, FitsTable, write_fits

        table = FitsTable(
            {
                "means": self.means_numpy.astype(np.float64),
                "weights": self.weights_numpy.astype(np.float64),
                "covariances": self.covariances_numpy.astype(np.float64),
            },
            meta={"PNPTYPE": self.meta.patch_norm.to_dict()["type"]},
        )
        write_fits(filename, [HDU(kind="primary"), HDU(table, name="GMM")], overwrite=overwrite)

    # fitting -------------------------------------------------------------------------------
    @classmethod
    def fit(cls, patches, n_components=None, *, init=None, means_init=None, covariances_init=None, weights_init=None,
            n_iter=100, tol=1e-3, reg_covar=1e-6, random_state=0, meta=None, init_params=None, kmeans_iter=100,
            kmeans_seed_patches=None):
        """Fit a full-covariance mixture to ``patches`` by EM on the GPU, with the steps of
        ``sklearn.mixture.GaussianMixture(covariance_type="full")``.

        patches : HIP float32 tensor (n, D), D = 64 or 256, already normalised (see `fit_images`).
        The start is a model ``init``, or the three arrays ``means_init`` (K, D), ``covariances_init`` (K, D, D) and
        ``weights_init`` (K,), or -- with ``n_components`` alone -- K distinct patches drawn by
        ``numpy.random.RandomState(random_state)`` as means, the covariance of all patches + ``reg_covar`` I for every
        component and uniform weights (``init_params="random-patches"``, the default).  ``init_params="kmeans"`` is
        scikit-learn's default scheme instead: `kmeans` clusters the patches (k-means++ seeds from
        ``RandomState(random_state)`` on ``kmeans_seed_patches`` patches, at most ``kmeans_iter`` Lloyd steps on the device),
        and the clusters' weights, means and covariances + ``reg_covar`` I -- one pass of hard assignments,
        `jd_gmm_fit_step_labels`, finished by `em_m_step` -- start EM.  A cluster of fewer than D patches cannot carry a
        covariance: ValueError.  Both starts are deterministic; neither draws scikit-learn's random numbers, so the two
        packages agree step by step only from a common explicit start.  ``init_params`` cannot be combined with a given
        start.

        Every step is one pass of the device over the patches (csrc/gmm_fit.hip: responsibilities, and the weighted
        moments about the current means); the division, the mean correction, the ridge and the Cholesky factors are done
        on the host in float64 and K D^2 floats are uploaded.  The iteration stops when the mean log-likelihood changes by
        less than ``tol`` or after ``n_iter`` steps.  A component whose weight sum falls below D cannot carry a
        covariance: ValueError names it.

        Returns a model built by `from_numpy` from the float64 result, carrying ``meta`` and a ``fit_info`` dict with
        ``lower_bounds`` (one per step), ``converged``, ``n_iter`` and the float64 ``means``, ``covariances``, ``weights``;
        after the k-means start also ``kmeans``: its ``inertia`` per Lloyd step, ``n_iter``, ``converged``, ``counts`` and
        the start it produced (``means``, ``covariances``, ``weights``)."""
        from ...ops import GmmFitHandle

        given = [a is not None for a in (means_init, covariances_init, weights_init)]
        if init_params is not None:
            if init_params not in ("random-patches", "kmeans"):
                raise ValueError(f'init_params is "random-patches" or "kmeans", got {init_params!r}')
            if init is not None or any(given):
                raise ValueError("init_params selects a start of its own: it cannot be given with `init` or *_init arrays")
        if init is not None and any(given):
            raise ValueError("give either `init` or means_init / covariances_init / weights_init, not both")
        if any(given) and not all(given):
            raise ValueError("means_init, covariances_init and weights_init are given together or not at all")
        if not isinstance(patches, torch.Tensor) or patches.ndim != 2 or patches.dtype != torch.float32:
            raise ValueError("patches must be a float32 torch tensor of shape (n, D)")
        n, D = int(patches.shape[0]), int(patches.shape[1])
        if D not in (64, 256):
            raise ValueError(f"patches of D = 64 or D = 256 features only, got D = {D}")
        if n < 1 or n > (2**31 - 1) // D:
            raise ValueError(f"1 <= n <= (2^31 - 1) / D patches, got n = {n}")
        if init is not None:
            means = init.means_numpy.astype(np.float64)
            covariances = init.covariances_numpy.astype(np.float64)
            weights = init.weights_numpy.astype(np.float64)
        elif all(given):
            means = np.array(means_init, dtype=np.float64)
            covariances = np.array(covariances_init, dtype=np.float64)
            weights = np.array(weights_init, dtype=np.float64)
        else:
            means = covariances = weights = None
        if means is not None:
            K = means.shape[0] if means.ndim == 2 else -1
            if means.shape != (K, D) or covariances.shape != (K, D, D) or weights.shape != (K,):
                raise ValueError(
                    f"start of shapes {means.shape}, {covariances.shape}, {weights.shape} does not fit (K, {D}), (K, {D}, {D}), (K,)"
                )
            if n_components is not None and int(n_components) != K:
                raise ValueError(f"n_components = {n_components} but the start has {K} components")
        else:
            if n_components is None:
                raise ValueError("n_components is needed without a start")
            K = int(n_components)
            if K > n:
                raise ValueError(f"{K} distinct patches as means need n >= {K}, got n = {n}")
        if not 1 <= K <= 1024:
            raise ValueError(f"1 <= n_components <= 1024, got {K}")
        if int(n_iter) < 1:
            raise ValueError("n_iter must be at least 1")
        if not patches.is_cuda:
            raise RuntimeError("patches must be a HIP tensor: jolideco_amd has no CPU path")
        patches = patches.contiguous()
        device = patches.device

        handle = _fit_handle(GmmFitHandle, device, D, K)
        kmeans_info = None
        if means is None and init_params == "kmeans":
            means, covariances, weights, kmeans_info = kmeans_start(handle, patches, K, reg_covar, random_state, kmeans_iter,
                                                                    kmeans_seed_patches)
        elif means is None:
            means, covariances, weights = random_start(patches, K, reg_covar, random_state)

        lower_bounds, converged = [], False
        previous = -np.inf
        for _ in range(int(n_iter)):
            means, covariances, weights, lower_bound, sum_r = em_step(handle, patches, means, covariances, weights, reg_covar)
            starved = np.flatnonzero(~(sum_r >= D))
            if starved.size:
                raise ValueError(
                    f"component {int(starved[0])} is starved: its responsibilities sum to {sum_r[starved[0]]:.3g}, fewer than "
                    f"the D = {D} patches a covariance needs (components {starved.tolist()}); choose another start or fewer components"
                )
            lower_bounds.append(lower_bound)
            if abs(lower_bound - previous) < tol:
                converged = True
                break
            previous = lower_bound
        model = cls.from_numpy(means, covariances, weights, meta=meta)
        # (the float64 parameters as well: the model's own arrays are their float32 roundings)
        model.fit_info = {"lower_bounds": lower_bounds, "converged": converged, "n_iter": len(lower_bounds),
                          "means": means, "covariances": covariances, "weights": weights}
        if kmeans_info is not None:
            model.fit_info["kmeans"] = kmeans_info
        return model

    @classmethod
    def fit_images(cls, images, patch_shape=(8, 8), stride=None, patch_norm=None, **fit_kwargs):
        """`fit` on the overlapping patches of HIP images: one (H, W) tensor, a (B, H, W) tensor or a list of images.

        The patches are cut with ``unfold`` at ``stride`` (default: half the patch edge); those that fail the prior's own
        ``> -1e5`` filter or hold non-finite values, before or after the norm, are dropped; ``patch_norm`` (default:
        subtract-mean) is applied in its host form.  The result's ``meta`` holds the stride and the patch norm, so it goes
        into ``GMMPatchPrior(gmm=...)`` and `write` as it is."""
        if "meta" in fit_kwargs:
            raise ValueError("fit_images sets `meta` itself (stride and patch norm)")
        ph, pw = (int(v) for v in patch_shape)
        if ph != pw or ph * pw not in (64, 256):
            raise ValueError(f"patch_shape (8, 8) or (16, 16) only, got {tuple(patch_shape)}")
        stride = ph // 2 if stride is None else int(stride)
        if stride < 1:
            raise ValueError("stride must be positive")
        patch_norm = SubtractMeanPatchNorm() if patch_norm is None else patch_norm
        if isinstance(images, torch.Tensor):
            images = [images] if images.ndim == 2 else list(images)
        rows = []
        for image in images:
            if not (isinstance(image, torch.Tensor) and image.is_cuda):
                raise RuntimeError("images must be HIP tensors: jolideco_amd has no CPU path")
            if image.ndim != 2 or image.shape[0] < ph or image.shape[1] < pw:
                raise ValueError(f"every image must be 2-d and at least {ph} x {pw}, got {tuple(image.shape)}")
            cut = image.to(torch.float32).unfold(0, ph, stride).unfold(1, pw, stride).reshape(-1, ph * pw)
            cut = cut[((cut > -1e5) & torch.isfinite(cut)).all(dim=1)]  # patches/core.py:215
            normed = patch_norm(cut)
            rows.append(normed[torch.isfinite(normed).all(dim=1)])
        if not rows:
            raise ValueError("no images")
        patches = torch.cat(rows).contiguous()
        meta = GaussianMixtureModelMeta(stride=stride, patch_norm=patch_norm)
        return cls.fit(patches, meta=meta, **fit_kwargs)

    @property
    def n_components(self):
        return self.covariances_numpy.shape[0]

    @property
    def n_features(self):
        return self.covariances_numpy.shape[1]

    @property
    def patch_shape(self):
        npix = int(self.means_numpy.shape[-1] ** 0.5)
        return npix, npix

    @property
    def eigen_images(self):
        """(K, P, P) float64, cached: per component ``w, v = numpy.linalg.eigh(cov_k)`` in float64 and ``(v @ w)``, the
        eigenvectors summed with their eigenvalues as weights, as a patch (patches/gmm.py:170-182) -- the default table of
        `GMMPatchPrior.prior_image`.  The signs of the eigenvectors are LAPACK's, so the table is defined up to them; its
        norm is not: ``|eigen_image_k|_2 = |cov_k|_F``."""
        if self._eigen_images is None:
            images = []
            for cov in self.covariances_numpy.astype(np.float64):
                w, v = np.linalg.eigh(cov)
                images.append((v @ w).reshape(self.patch_shape))
            self._eigen_images = np.stack(images)
        return self._eigen_images

    def reduce_to_topk(self, k):
        """The mixture of the ``k`` components of largest weight, in descending order of weight, with their means and
        covariances and this model's meta (patches/gmm.py:391-411; the weights are not renormalised, as there)."""
        idx = np.argsort(self.weights_numpy)[::-1][:k]
        return self.__class__.from_numpy(
            means=self.means_numpy[idx], covariances=self.covariances_numpy[idx], weights=self.weights_numpy[idx], meta=self.meta
        )

    def is_equal(self, other):
        """The covariances have one shape and are close (`numpy.allclose`): patches/gmm.py:447-452."""
        if self.covariances_numpy.shape != other.covariances_numpy.shape:
            return False
        return bool(np.allclose(self.covariances_numpy, other.covariances_numpy))

    # fp32 constants, computed with the same fp32 torch ops as the reference ------------------
    @property
    def means_precisions_cholesky_numpy(self):
        """mu_k @ P_k in fp32 (gmm.py:217-228)."""
        mu = torch.from_numpy(self.means_numpy)
        pc = torch.from_numpy(self.precisions_cholesky_numpy)
        return torch.stack([torch.matmul(m, p) for m, p in zip(mu, pc)]).numpy()

    @property
    def log_det_cholesky_numpy(self):
        """sum_i log P_k[i, i] in fp32 (gmm.py:235-240)."""
        pc = torch.from_numpy(self.precisions_cholesky_numpy)
        diag = pc.reshape(self.n_components, -1)[:, :: self.n_features + 1]
        return torch.sum(torch.log(diag), axis=1).numpy()

    @property
    def const_float64_numpy(self):
        """-D/2 log(2 pi) + sum_i log P_k[i, i] + log pi_k of the float32 factors and weights, evaluated in float64 (K,):
        the constants of `estimate_log_prob` without the roundings of their float32 sum (`ops.GmmHandle`)."""
        pc = self.precisions_cholesky_numpy.astype(np.float64)
        diag = pc.reshape(self.n_components, -1)[:, :: self.n_features + 1]
        log_weights = np.log(self.weights_numpy.astype(np.float64))
        return -0.5 * self.n_features * np.log(2 * np.pi) + np.log(diag).sum(axis=1) + log_weights

    @property
    def log_weights_numpy(self):
        return torch.log(torch.from_numpy(self.weights_numpy)).numpy()

    @property
    def pixel_weights_numpy(self):
        """(1, D) overlap weights; all ones when ``meta.stride`` is None (gmm.py:290-299)."""
        if self.meta.stride is None:
            weights = np.ones(self.patch_shape)
        else:
            weights = get_pixel_weights(patch_shape=self.patch_shape, stride=self.meta.stride)
        return weights.reshape((1, -1))

    # device side ---------------------------------------------------------------------------
    def handle(self, device):
        """Native handle for ``device`` (created on first use, cached)."""
        from ...ops import GmmHandle

        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = str(device)
        if key not in self._handles:
            self._handles[key] = GmmHandle(
                precisions_cholesky=self.precisions_cholesky_numpy,
                means_precisions_cholesky=self.means_precisions_cholesky_numpy,
                log_det_cholesky=self.log_det_cholesky_numpy,
                log_weights=self.log_weights_numpy,
                pixel_weights=self.pixel_weights_numpy.astype(np.float32),
                device=device,
                const_float64=self.const_float64_numpy,
            )
        return self._handles[key]

    def estimate_log_prob(self, x):
        """(n, K) weighted log-probabilities of already normalised patches ``x`` (n, D) on the GPU
        (jolideco/priors/patches/gmm.py:262-281)."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise RuntimeError("x must be a HIP tensor: jolideco_amd has no CPU path")
        return self.handle(x.device).estimate_log_prob(x.contiguous())

    def __deepcopy__(self, memo):
        # constants are immutable: share them (and the native handles) between copies
        return self

    def to_dict(self):
        """``{"type": <name in the GMM library>}`` like the reference (gmm.py:458-471); a model built from
        explicit arrays has no name and is recorded as "custom" with its size."""
        if self.registry_name is not None:
            return {"type": self.registry_name}
        return {"type": "custom", "n_components": int(self.n_components), "n_features": int(self.n_features)}

    @classmethod
    def from_dict(cls, data):
        return cls.from_registry(name=data["type"])

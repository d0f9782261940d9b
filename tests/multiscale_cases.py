"""Shared by tools/make_golden_multiscale.py, tests/test_multiscale_golden.py (CPU) and tests/test_gpu_multiscale.py (GPU):
the cases of `MultiScalePrior` and a CPU restatement of what the reference computes
(jolideco/priors/patches/core.py:249-337), in torch, float32 or float64, composed from `oracle.cpu_ref.gmm_patch_log_prior`,
a direct zero-padded convolution and an average pooling:

    g = flux                                   (1, 1, H, W); rolled by the outer draw when cycle_spin is on
    for l = 0 .. L-1, f = 2^l:
        if w_l == 0: continue                  (the blur of the level is skipped too)
        if anti_alias: g = K_l (*) g           K_l = Gaussian of sigma 2 f / 6, "same", zero padded, cumulative
        value += f^2 * w_l * prior(avg_pool2d(g, f))

The reference convolves through an FFT.  With `conv_same_fft` the float32 restatement reproduces it bit for bit
(tools/make_golden_multiscale.py asserts that on every case the reference can run); the tests use the direct sum of the
taps (`conv_same_direct`, the default), which is what the kernels do and has the smaller float32 error.  With the
outer ``cycle_spin=True`` the reference raises, so those cases exist in the restatement only.

The mixtures are synthetic and never stored: `cpu_ref.synthetic_gmm(K, D, seed, zero_means=False)` rounded to float32,
rebuilt here from (K, D, seed); the fixture holds a float64 checksum of the ones it was generated with."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref

ASINH = {"alpha": 3.0, "beta": 40.0}
MAX_LEVELS = 5

_BASE = dict(n_levels=2, weights=None, anti_alias=True, marginalize=False, norm=None, inner_spin=False, inner_seed=None,
             outer_spin=False, D=64, K=5, stride=4, gmm_seed=4101, flux_seed=4201)


def _case(shape, **kwargs):
    return dict(_BASE, shape=shape, **kwargs)


# name -> settings.  The seeds are chosen so that the float64 arg-max margins are clear (see `margins`, and the fixture).
CASES = {
    "32x40-L1": _case((32, 40), n_levels=1),
    "32x40-L2": _case((32, 40), n_levels=2),
    "32x40-L3": _case((32, 40), n_levels=3),
    "33x41-L2": _case((33, 41), n_levels=2, flux_seed=4202),
    "33x41-L3": _case((33, 41), n_levels=3, flux_seed=4202),
    "48x48-L3": _case((48, 48), n_levels=3, flux_seed=4203),
    "skip-level": _case((32, 40), n_levels=3, weights=[0.6, 0.0, 0.4]),
    "no-anti-alias": _case((32, 40), n_levels=2, anti_alias=False),
    "marginalize": _case((32, 40), n_levels=2, marginalize=True),
    "asinh": _case((32, 40), n_levels=2, norm="asinh"),
    "inner-spin": _case((33, 41), n_levels=3, inner_spin=True, inner_seed=4301, flux_seed=4202),
    "gmm16": _case((48, 48), n_levels=2, D=256, K=3, stride=8, gmm_seed=4102, flux_seed=4203),
    "outer-spin": _case((33, 41), n_levels=3, outer_spin=True, inner_spin=False, inner_seed=4302, flux_seed=4202),
    "outer-inner-spin": _case((32, 40), n_levels=2, outer_spin=True, inner_spin=True, inner_seed=4303),
}
REFERENCE_CASES = [name for name, case in CASES.items() if not case["outer_spin"]]  # (the reference raises on the others)

FIT = dict(shape=(32, 32), n_epochs=6, n_levels=2, K=5, D=64, stride=4, gmm_seed=4103, seed=4401)


@functools.lru_cache(maxsize=None)
def synthetic_mixture(k, d, seed):
    """(means, covariances, weights) as float64 arrays holding float32 values"""
    arrays = cpu_ref.synthetic_gmm(k, d, seed=seed, zero_means=False)
    return tuple(np.asarray(a, dtype=np.float32).astype(np.float64) for a in arrays)


def mixture_checksum(arrays):
    means, covs, weights = arrays
    ramp = 1.0 + np.arange(covs.size, dtype=np.float64).reshape(covs.shape) / covs.size  # (position sensitive)
    return float(np.sum(covs * ramp) + np.sum(means) + np.sum(weights * np.arange(1, weights.size + 1)))


def case_mixture(case):
    return synthetic_mixture(case["K"], case["D"], case["gmm_seed"])


def case_flux(case):
    return np.random.RandomState(case["flux_seed"]).gamma(20, size=case["shape"]).astype(np.float32)


def level_weights(n_levels, weights=None):
    """softmax of the log-weights in float32, as the reference forms them (core.py:277-286)"""
    w = torch.tensor([1 / n_levels] * n_levels) if weights is None else torch.as_tensor(weights, dtype=torch.float32)
    log_w = torch.log(w)
    return torch.exp(log_w) / torch.sum(torch.exp(log_w))


def gaussian_kernel(sigma):
    """float64 array of astropy's ``Gaussian2DKernel(sigma)``: sampled at the pixel centres on an odd number of pixels
    >= 8 sigma, normalised to sum 1 (asserted against the reference's own array when the fixture is written)."""
    size = int(np.ceil(8 * sigma))
    size += 1 - size % 2
    axis = np.arange(size, dtype=float) - size // 2
    x, y = np.meshgrid(axis, axis)
    array = 1.0 / (2 * np.pi * sigma**2) * np.exp(-0.5 * (x**2 + y**2) / sigma**2)
    return array / array.sum()


def level_kernel(level):
    """the float32 kernel the reference convolves with at `level` (core.py:316-319)"""
    return gaussian_kernel(2 * 2**level / 6.0).astype(np.float32)


def conv_same_direct(image, kernel):
    """"same" zero-padded linear convolution of a (1, 1, H, W) tensor with an odd square kernel, summed tap by tap"""
    r = kernel.shape[-1] // 2
    return F.conv2d(image, torch.flip(kernel, dims=(-2, -1))[None, None], padding=r)


def make_norm(case):
    if case["norm"] is None:
        return None
    from jolideco_amd.utils.norms import NORMS_REGISTRY

    return NORMS_REGISTRY[case["norm"]](**ASINH)


def draws(case):
    """The draws of one evaluation in the reference's order: (outer roll | None, one entry per level: the inner prior's
    roll | None), from a generator seeded with the case's ``inner_seed`` (the inner prior's generator serves both)."""
    generator = torch.Generator(device="cpu")
    if case["inner_seed"] is not None:
        generator.manual_seed(case["inner_seed"])
    p = int(round(case["D"] ** 0.5))
    return draws_from(generator, case["n_levels"], case["weights"], case["outer_spin"], case["inner_spin"], (p, p))


def draws_from(generator, n_levels, weights, outer_spin, inner_spin, patch_shape):
    w = level_weights(n_levels, weights)
    outer = cpu_ref.draw_cycle_spin_shifts(generator, patch_shape) if outer_spin else None
    inner = tuple(cpu_ref.draw_cycle_spin_shifts(generator, patch_shape) if (inner_spin and w[level] != 0) else None
                  for level in range(n_levels))
    return (outer,) + inner


def conv_same_fft(image, kernel):
    """the reference's own route (`cpu_ref.convolve_fft` restates `convolve_fft_torch`): with it the float32 restatement
    reproduces the reference bit for bit, which tools/make_golden_multiscale.py asserts"""
    return cpu_ref.convolve_fft(image, kernel[None, None])


def multiscale_log_prior(flux, gmm, stride, shifts, n_levels, weights=None, anti_alias=True, marginalize=False, norm=None,
                         details=None, conv=conv_same_direct):
    """The restatement: scalar tensor (differentiable with respect to ``flux``, a (1, 1, H, W) tensor in the working
    precision).  ``shifts``: as `draws` returns them.  ``details``: a list that receives, per evaluated level, a dict with
    the pooled image and the (patches, K) log-likelihoods."""
    w = level_weights(n_levels, weights)
    g = flux
    if shifts[0] is not None:
        g = torch.roll(g, shifts=tuple(int(s) for s in shifts[0]), dims=(2, 3))
    value = 0
    for level in range(n_levels):
        f = 2**level
        if w[level] == 0:
            continue
        if anti_alias:
            g = conv(g, cpu_ref._tensor(level_kernel(level)))
        pooled = F.avg_pool2d(g, kernel_size=f)
        image = pooled if norm is None else norm(pooled)
        value_level = cpu_ref.gmm_patch_log_prior(image, gmm, stride, shifts[1 + level], marginalize)
        # (f**2 * w_l is the reference's float32 product; in float64 the same float32 number, widened)
        value = value + (f**2 * w[level]).to(flux.dtype) * value_level
        if details is not None:
            loglike = cpu_ref.gmm_patch_log_like(image.detach(), gmm, stride, shifts[1 + level])
            details.append({"level": level, "pooled": pooled.detach().numpy()[0, 0], "image": image.detach().numpy()[0, 0],
                            "loglike": loglike.numpy()})
    return value


class MultiScalePriorRef:
    """Callable for `cpu_ref.map_fit_sequential` / `map_fit_joint`: one draw per evaluation from the inner prior's
    generator (torch's default seed unless given), like the reference's inner `GMMPatchPrior`."""

    def __init__(self, gmm, stride, n_levels=2, weights=None, outer_spin=False, inner_spin=True, anti_alias=True,
                 marginalize=False, generator=None, conv=conv_same_direct):
        self.gmm, self.stride, self.n_levels, self.weights, self.conv = gmm, stride, n_levels, weights, conv
        self.outer_spin, self.inner_spin, self.anti_alias, self.marginalize = outer_spin, inner_spin, anti_alias, marginalize
        self.generator = generator if generator is not None else torch.Generator(device="cpu")
        self.last_shifts = None

    def __call__(self, flux):
        self.last_shifts = draws_from(self.generator, self.n_levels, self.weights, self.outer_spin, self.inner_spin,
                                      self.gmm.patch_shape)
        return multiscale_log_prior(flux, self.gmm, self.stride, self.last_shifts, self.n_levels, self.weights, self.anti_alias,
                                    self.marginalize, conv=self.conv)


def fit_inputs():
    """(datasets, flux_init, mixture arrays) of the fit case: two observations of a 32 x 32 scene"""
    rs = np.random.RandomState(FIT["seed"])
    h, w = FIT["shape"]
    y, x = np.mgrid[0:h, 0:w].astype(float)
    truth = 2.0 + 40 * np.exp(-0.5 * (((y - h * 0.4) / (h / 9)) ** 2 + ((x - w * 0.55) / (w / 7)) ** 2))
    for _ in range(4):
        truth[rs.randint(0, h), rs.randint(0, w)] += rs.uniform(100, 800)
    datasets = {}
    for i in range(2):
        axis = np.arange(7) - 3.0
        psf = np.exp(-0.5 * (axis[:, None] ** 2 / (1.5 + 0.5 * i) ** 2 + (axis[None, :] + 0.4) ** 2 / 2.0**2))
        psf /= psf.sum()
        exposure = (1 + 0.5 * np.linspace(-1, 1, h)).reshape(-1, 1) * (1 + 0.2 * np.linspace(-1, 1, w))
        padded = np.pad(truth * exposure, 3)
        npred = sum(psf[3 - dy, 3 - dx] * padded[3 + dy : 3 + dy + h, 3 + dx : 3 + dx + w]
                    for dy in range(-3, 4) for dx in range(-3, 4)) + 0.8
        datasets[f"o{i}"] = {"counts": rs.poisson(npred).astype(np.float32), "psf": psf.astype(np.float32),
                             "exposure": exposure.astype(np.float32), "background": np.full((h, w), 0.8, dtype=np.float32)}
    flux_init = rs.gamma(30, size=FIT["shape"])
    return datasets, flux_init, synthetic_mixture(FIT["K"], FIT["D"], FIT["gmm_seed"])


def restate(case, dtype=np.float32, flux_np=None, shifts=None, conv=conv_same_direct):
    """{value, grad (float64 array), levels: [details]} of a case in `dtype`"""
    shifts = draws(case) if shifts is None else shifts
    flux_np = case_flux(case) if flux_np is None else flux_np
    with cpu_ref.precision(dtype):
        gmm = cpu_ref.GMM.from_numpy(*case_mixture(case), stride=case["stride"])
        flux = cpu_ref._tensor(flux_np[np.newaxis, np.newaxis]).requires_grad_(True)
        details = []
        value = multiscale_log_prior(flux, gmm, case["stride"], shifts, case["n_levels"], case["weights"], case["anti_alias"],
                                     case["marginalize"], make_norm(case), details, conv)
        value.backward()
        return {"value": float(value.detach()), "grad": flux.grad.numpy()[0, 0].astype(np.float64), "levels": details}


@functools.lru_cache(maxsize=None)
def cached_restate(name, dtype_name):
    return restate(CASES[name], np.dtype(dtype_name).type)


def margins(levels):
    """best minus runner-up log-likelihood of every patch of every level (float64 details), concatenated"""
    out = []
    for level in levels:
        top = np.sort(np.asarray(level["loglike"], dtype=np.float64), axis=1)
        out.append(top[:, -1] - top[:, -2])
    return np.concatenate(out)


def mean_free_patches(image, p, stride, shifts):
    """(N, p*p) float64: the patches of the (rolled) image minus their means, as the prior extracts them"""
    t = torch.from_numpy(np.asarray(image, dtype=np.float64))
    if shifts is not None:
        t = torch.roll(t, shifts=tuple(int(s) for s in shifts), dims=(0, 1))
    x = cpu_ref.overlapping_patches(t, p, stride)
    return (x - x.mean(dim=1, keepdim=True)).numpy()


# ---- the kernels alone: float64 / float32 numpy evaluations of the same separable formula ------------------------------------
def down_numpy(x, f, taps, shifts=None, dtype=np.float64):
    """(g, d): g = outer(taps, taps) (*) x ("same", zero padded; x rolled by `shifts` first), d = its f x f means (floor),
    all sums in `dtype`: the row pass, then the column pass, then the cell's rows left to right and top to bottom"""
    x = np.asarray(x, dtype=dtype)
    if shifts is not None:
        x = np.roll(x, shifts, axis=(0, 1))
    u = np.asarray(taps, dtype=dtype)
    H, W = x.shape
    r = len(u) // 2
    padded = np.zeros((H + 2 * r, W + 2 * r), dtype=dtype)
    padded[r : r + H, r : r + W] = x
    mid = np.zeros((H + 2 * r, W), dtype=dtype)
    for k in range(len(u)):  # convolution: tap k multiplies x[.., x - (k - r)]
        mid += u[k] * padded[:, 2 * r - k : 2 * r - k + W]
    g = np.zeros((H, W), dtype=dtype)
    for k in range(len(u)):
        g += u[k] * mid[2 * r - k : 2 * r - k + H, :]
    Hp, Wp = H // f, W // f
    cells = g[: Hp * f, : Wp * f].reshape(Hp, f, Wp, f)
    rows = np.zeros((Hp, f, Wp), dtype=dtype)
    for j in range(f):
        rows += cells[:, :, :, j]
    d = np.zeros((Hp, Wp), dtype=dtype)
    for j in range(f):
        d += rows[:, j, :]
    return g, d * dtype(1.0 / (f * f))


def up_numpy(dd, dg, shape, f, taps, dtype=np.float64):
    """K^T (*) (dg + replicate_f(dd) / f^2) on `shape` (correlation with outer(taps, taps), zero padded), in `dtype`"""
    H, W = shape
    u = np.asarray(taps, dtype=dtype)
    r = len(u) // 2
    t = np.zeros((H, W), dtype=dtype)
    Hp, Wp = H // f, W // f
    t[: Hp * f, : Wp * f] = np.repeat(np.repeat(np.asarray(dd, dtype=dtype), f, axis=0), f, axis=1) * dtype(1.0 / (f * f))
    if dg is not None:
        t = t + np.asarray(dg, dtype=dtype)
    padded = np.zeros((H + 2 * r, W + 2 * r), dtype=dtype)
    padded[r : r + H, r : r + W] = t
    mid = np.zeros((H + 2 * r, W), dtype=dtype)
    for k in range(len(u)):
        mid += u[k] * padded[:, k : k + W]
    out = np.zeros((H, W), dtype=dtype)
    for k in range(len(u)):
        out += u[k] * mid[k : k + H, :]
    return out


def kernel_taps(n_taps, seed):
    """n_taps positive float32 factors, deliberately NOT symmetric (a flipped pass would show), summing to about 1"""
    rs = np.random.RandomState(seed)
    u = np.exp(-0.5 * ((np.arange(n_taps) - n_taps // 2) / max(n_taps / 6.0, 0.5)) ** 2) * rs.uniform(0.7, 1.3, n_taps)
    return (u / u.sum()).astype(np.float32) if n_taps > 1 else np.ones(1, dtype=np.float32)


# (shape, f, taps): cross a tile boundary (32 x 64 tiles), ragged pooling cells, the halo outside the image on all four sides
KERNEL_CASES = [((33, 130), 1, 3), ((17, 23), 2, 7), ((40, 70), 4, 11), ((24, 72), 8, 23), ((48, 80), 16, 43), ((33, 41), 2, 1)]

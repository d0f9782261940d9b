"""Shared by tests/test_priors_golden.py (CPU) and tests/test_gpu_priors.py (GPU): the cases of the sub-pixel cycle spin of
the sparse priors and of the smoothness prior, and their CPU oracles in float32 / float64 (numpy / torch only; pinned against
the live reference when tools/make_golden_priors.py generated tests/golden/priors.npz)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref

KINDS = {"inverse-gamma": 1, "exponential": 2}
# constructor arguments of the fixture's priors
SPARSE_PARAMS = {"inverse-gamma": {"alpha": 10.0, "beta": 1.5}, "exponential": {"alpha": 10.0}}
FIXTURE_SHAPE = (24, 40)
FIXTURE_SEED = 1811          # the seeded CPU generator of the fixture's sparse priors
SMOOTH_WIDTHS = (2, 1.5)
FIT_SHAPE, FIT_EPOCHS, FIT_SEED = (32, 32), 6, 77

# sub-pixel kernel: smaller than a tile | one row / one column | one past a tile edge (tiles are 32 x 64) | whole tiles,
# vector path | odd pitch, unaligned rows
SUBPIX_SHAPES = [(5, 7), (1, 40), (40, 1), (33, 65), (64, 96), (37, 53)]
# all four sign quadrants, no shift, the corner of the range (|t - o| = 1 - 2^-25 rounds: weights at the edge of float32)
SUBPIX_OFFSETS = [(0.3, 0.2), (-0.25, 0.4), (0.125, -0.45), (-0.4, -0.15), (0.0, 0.0), (-0.5, 0.49999997)]
# smoothness prior: (shape, width) -- kernel (17 x 17) larger than the image | several tiles | odd sizes
SMOOTH_CASES = [((9, 9), 2), ((40, 56), 2), ((65, 33), 2)]


def fixture_flux():
    return np.random.RandomState(1234).gamma(2.0, size=FIXTURE_SHAPE).astype(np.float32)


def case_flux(shape, seed=0):
    """Gamma-distributed positive flux (shape 2: a few values near zero, where the inverse-gamma terms are large)."""
    return (0.05 + np.random.RandomState(4100 + 131 * shape[0] + shape[1] + seed).gamma(2.0, size=shape)).astype(np.float32)


def subpix_kernel(x0, y0):
    """(3, 3) float32 weights of the reference's `grid_weights` for the offsets (x0, y0) -- its float32 operations."""
    grid = torch.arange(-1, 2)
    y, x = torch.meshgrid(grid, grid, indexing="ij")
    x0, y0 = torch.tensor([x0], dtype=torch.float32), torch.tensor([y0], dtype=torch.float32)
    dx = torch.abs(x - x0)
    dx = torch.where(dx < 1, 1 - dx, 0)
    dy = torch.abs(y - y0)
    dy = torch.where(dy < 1, 1 - dy, 0)
    return dx * dy


def draw_offsets(generator):
    """One pair (x0, y0) as the reference draws it: float32 `rand(1) - 0.5`, x first."""
    x0 = torch.rand(1, generator=generator) - 0.5
    y0 = torch.rand(1, generator=generator) - 0.5
    return float(x0), float(y0)


def log_constant(kind, alpha, beta):
    if kind == "inverse-gamma":
        return cpu_ref.InverseGammaPriorRef(alpha, beta).log_constant_term
    return float(cpu_ref.ExponentialPriorRef(alpha).log_constant_term)


def sparse_log_prior(flux, kind, alpha, beta, kernel, log_const):
    """The reference's formula on s = conv2d(flux, kernel, "same"), in the dtype of `flux` (alpha, beta: float32 values)."""
    s = F.conv2d(flux, kernel.to(flux.dtype).reshape(1, 1, 3, 3), padding="same")
    alpha, beta = torch.Tensor([alpha]).to(flux.dtype), torch.Tensor([beta]).to(flux.dtype)  # (float32 values, as stored)
    if kind == "inverse-gamma":
        value = -beta / s
        value += (-alpha - 1) * torch.log(s)
    else:
        value = -alpha * s
    return torch.sum(value) / flux.numel() + log_const


def sparse_oracle(flux_np, kind, x0, y0, dtype=np.float64, alpha=None, beta=None):
    """(value, gradient with respect to the flux) of a sparse prior with sub-pixel offsets (x0, y0), in `dtype`.  The
    weights are the float32 numbers the reference and the kernel use, in every precision."""
    params = dict(SPARSE_PARAMS[kind])
    alpha = params["alpha"] if alpha is None else alpha
    beta = params.get("beta", 0.0) if beta is None else beta
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    flux = torch.tensor(np.asarray(flux_np)[None, None], dtype=tdtype, requires_grad=True)
    value = sparse_log_prior(flux, kind, alpha, beta, subpix_kernel(x0, y0), log_constant(kind, alpha, beta))
    value.backward()
    return float(value.detach()), flux.grad.numpy()[0, 0].astype(np.float64)


@functools.lru_cache(maxsize=None)
def cached_sparse_oracle(shape, kind, offsets, dtype_name):
    return sparse_oracle(case_flux(shape), kind, *offsets, dtype=np.dtype(dtype_name).type)


class SubpixPriorRef:
    """The reference's InverseGammaPrior / ExponentialPrior with cycle_spin_subpix=True as a callable for
    `cpu_ref.map_fit_sequential`: draws (x0, y0) per evaluation from `generator` (default: torch's default seed)."""

    def __init__(self, kind, alpha=10, beta=3 / 2, generator=None):
        self.kind, self.alpha, self.beta = kind, alpha, beta
        self.log_const = log_constant(kind, alpha, beta)
        self.generator = generator if generator is not None else torch.Generator("cpu")
        self.drawn = []

    def __call__(self, flux):
        offsets = draw_offsets(self.generator)
        self.drawn.append(offsets)
        return sparse_log_prior(flux, self.kind, self.alpha, self.beta, subpix_kernel(*offsets), self.log_const)


def gaussian_kernel(width):
    """astropy's Gaussian2DKernel(width).array (>= 5.2): pixel centres, odd size >= 8 width, normalised to sum 1."""
    sigma = float(width)
    size = int(np.ceil(8 * sigma))
    size += 1 - size % 2
    axis = np.arange(size, dtype=float) - size // 2
    x, y = np.meshgrid(axis, axis)
    array = 1.0 / (2 * np.pi * sigma**2) * np.exp(-0.5 * (x**2 + y**2) / sigma**2)
    return array / array.sum()


class SmoothnessPriorRef:
    """The reference's SmoothnessPrior, operation by operation: -sum(flux * convolve_fft(flux, kernel)) with the float64
    kernel tensor (the product of the spectra, and everything after it, is then double precision)."""

    def __init__(self, width=2):
        self.kernel = torch.from_numpy(gaussian_kernel(width)[None, None])

    def __call__(self, flux):
        return -torch.sum(flux * cpu_ref.convolve_fft(flux, self.kernel))


def smoothness_oracle(flux_np, kernel_np, dtype=np.float64):
    """(value, gradient) of -sum(f * (K (*) f)) by direct summation ("same", zero padded) in `dtype`."""
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    flux = torch.tensor(np.asarray(flux_np)[None, None], dtype=tdtype, requires_grad=True)
    k = np.asarray(kernel_np)
    kernel = torch.tensor(k[::-1, ::-1].copy()[None, None], dtype=tdtype)  # conv2d correlates: flip for a convolution
    pad = (k.shape[0] // 2, k.shape[1] // 2)
    value = -torch.sum(flux * F.conv2d(flux, kernel, padding=pad))
    value.backward()
    return float(value.detach()), flux.grad.numpy()[0, 0].astype(np.float64)


@functools.lru_cache(maxsize=None)
def cached_smoothness_oracle(shape, width, dtype_name):
    return smoothness_oracle(case_flux(shape, seed=7), gaussian_kernel(width), np.dtype(dtype_name).type)


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def bound(own_error, floor=1e-6):
    """The project's rule: at most 4 x the float32 CPU oracle's own error against float64, floor 1e-6 (relative L-inf)."""
    return max(4.0 * own_error, floor)

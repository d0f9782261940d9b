"""A plain float64 statement of the (calibrated, up-sampled) likelihood step, for the tests of the HIP step kernels.

    loss = mean(n - c log(n + eps)) + stirling
    n    = sum_components clip(sum_pool_U(conv_same(shift(flux) * E, psf)), 0) + bkg * exp(log_norm)

in torch autograd on the CPU: jolideco/models/npred.py:160-261 with the calibration of :298-402 on the flux-grid arrays
the C entries take (include/jolideco_hip.h: jd_npred_poisson_calibrated_fwd_bwd).  tests/test_step_oracle.py pins it to
`oracle.cpu_ref.DatasetRef.loss`.

The shift is written out, not taken from grid_sample: four zero-padded, integer-translated copies of the image weighted by
w1 = s - floor(s) and w0 = 1 - w1 (s = U * shift, floor(s) a constant).  That is the function the kernels compute
(csrc/shift.hip:1-6) and it fixes the derivative at an exactly integer shift to the right-hand one, which the kernels take
(shift.hip:29-32) and which grid_sample leaves to the rounding of its normalised coordinates.
"""
import numpy as np
import torch
import torch.nn.functional as F

POISSON_EPS = 1e-25  # jolideco/loss.py:36
DIRECT_LIMIT = 5e7  # multiply-adds up to which conv_same runs as a direct sum (exact zeros stay exact), FFT beyond


def stirling_mean(counts):
    """mean([c > 1] (c log c - c + 0.5 log(2 pi c))): the flux-independent term of PoissonNLLLoss(full=True)."""
    c = np.asarray(counts, dtype=np.float64)
    safe = np.where(c > 1, c, 1.0)
    return float(np.where(c > 1, safe * np.log(safe) - safe + 0.5 * np.log(2 * np.pi * safe), 0.0).mean())


def translate(image, dy, dx):
    """out[i, j] = image[i + dy, j + dx], zero where that lies outside the image (integer dy, dx of any size)."""
    H, W = image.shape
    out = torch.zeros_like(image)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    out[max(0, -dy) : H - max(0, dy), max(0, -dx) : W - max(0, dx)] = image[max(0, dy) : H - max(0, -dy), max(0, dx) : W - max(0, -dx)]
    return out


def shift_explicit(image, shift_pixels):
    """Bilinear shift of an (H, W) image: out[i, j] = image(i + s_y, j + s_x) with zero padding, ``shift_pixels`` = tensor
    [s_x, s_y] in pixels of this grid (differentiable; the derivative at an integer shift is the right-hand one)."""
    floor = torch.floor(shift_pixels).detach()
    w1 = shift_pixels - floor
    w0 = 1 - w1
    fx, fy = int(floor[0]), int(floor[1])
    return (
        translate(image, fy, fx) * (w0[0] * w0[1]) + translate(image, fy, fx + 1) * (w1[0] * w0[1])
        + translate(image, fy + 1, fx) * (w0[0] * w1[1]) + translate(image, fy + 1, fx + 1) * (w1[0] * w1[1])
    )


def _fast_length(n):
    while True:
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def conv_same(image, psf, method="auto"):
    """out[y, x] = sum_ab image[y + oy - a, x + ox - b] psf[a, b] with (oy, ox) = ((kh - 1) // 2, (kw - 1) // 2) and zeros
    outside the image.  ``method``: "direct" | "fft" | "auto" (direct up to DIRECT_LIMIT multiply-adds)."""
    H, W = image.shape
    kh, kw = psf.shape
    oy, ox = (kh - 1) // 2, (kw - 1) // 2
    if method == "auto":
        method = "direct" if float(H) * W * kh * kw <= DIRECT_LIMIT else "fft"
    if method == "direct":
        padded = F.pad(image[None, None], (kw - 1 - ox, ox, kh - 1 - oy, oy))
        return F.conv2d(padded, torch.flip(psf, (0, 1))[None, None])[0, 0]
    size = (_fast_length(H + kh - 1), _fast_length(W + kw - 1))
    full = torch.fft.irfft2(torch.fft.rfft2(image, s=size) * torch.fft.rfft2(psf, s=size), s=size)
    return full[oy : oy + H, ox : ox + W]


def sum_pool(image, U):
    H, W = image.shape
    return image.reshape(H // U, U, W // U, U).sum(dim=(1, 3)) if U > 1 else image


def step_oracle(flux, exposure, psf, background, counts, U, shift=None, log_norm=None, dtype=torch.float64, conv="auto"):
    """The step of one dataset.  ``flux`` / ``exposure`` / ``psf``: arrays on the flux grid (U x the counts grid; the PSF
    up-sampled and normalised as the caller wants it), or equally long lists of them for several flux components;
    ``background`` / ``counts``: counts-grid arrays; ``shift``: None or (shift_x, shift_y) in COUNTS pixels; ``log_norm``:
    None or the log of the background norm.

    Returns a dict of numpy values: ``loss``, ``grad_flux`` (array, or list for a list of components), ``grad_shift``
    ([d/d shift_x, d/d shift_y] or None), ``grad_log_norm`` (float or None), ``pooled`` (the pooled convolutions before
    the clip, per component: list of arrays), ``npred`` (n on the counts grid)."""
    single = not isinstance(flux, (list, tuple))
    fluxes, exposures, psfs = ([flux], [exposure], [psf]) if single else (list(flux), list(exposure), list(psf))
    as_t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)  # noqa: E731
    fl = [as_t(f).requires_grad_(True) for f in fluxes]
    s = None if shift is None else as_t(shift).requires_grad_(True)
    ln = None if log_norm is None else as_t(float(log_norm)).requires_grad_(True)
    c, bkg = as_t(counts), as_t(background)
    n = bkg * torch.exp(ln) if ln is not None else bkg
    pooled = []
    for f, e, p in zip(fl, exposures, psfs):
        shifted = shift_explicit(f, U * s) if s is not None else f
        pooled.append(sum_pool(conv_same(shifted * as_t(e), as_t(p), conv), U))
        n = n + torch.clip(pooled[-1], min=0)
    loss = (n - c * torch.log(n + POISSON_EPS)).mean() + stirling_mean(counts)
    loss.backward()
    grads = [f.grad.numpy() if f.grad is not None else np.zeros(f.shape) for f in fl]  # (None: the image was shifted out)
    return {
        "loss": float(loss.detach()),
        "grad_flux": grads[0] if single else grads,
        "grad_shift": None if s is None else (s.grad.numpy() if s.grad is not None else np.zeros(2)),
        "grad_log_norm": None if ln is None else float(ln.grad),
        "pooled": [p.detach().numpy() for p in pooled],
        "npred": n.detach().numpy(),
    }


def clip_margin(pooled):
    """Smallest ratio to the maximum among the pooled convolutions that are not zero (<= 1e-12 of the maximum): the clip
    is a kink, so a case is only meaningful where no counts pixel sits near it (ratio >= 1e-3)."""
    ratios = []
    for p in pooled:
        top = np.abs(p).max()
        if top == 0:
            continue
        r = np.abs(p) / top
        live = r[r > 1e-12]
        ratios.append(live.min() if live.size else np.inf)
    return min(ratios) if ratios else np.inf

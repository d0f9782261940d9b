"""Tensor utilities with the reference's names (jolideco/utils/torch.py), backed by the HIP library."""
import logging

import torch

__all__ = [
    "TORCH_DEFAULT_DEVICE",
    "convolve_fft_torch",
    "cycle_spin_shifts",
    "cycle_spin",
    "subpixel_offsets",
    "subpixel_offsets_many",
    "subpixel_kernel",
    "jitter_grid",
    "jitter_stride_check",
    "jitter_draws",
    "get_default_generator",
    "view_as_overlapping_patches_torch",
]

log = logging.getLogger(__name__)

# The reference defaults to "cpu" (utils/torch.py:21); this package only runs on the accelerator.
TORCH_DEFAULT_DEVICE = "cuda"


def convolve_fft_torch(image, kernel):
    """'same' FFT convolution of a (1, 1, H, W) image with a (1, 1, kh, kw) kernel on the GPU
    (rocFFT R2C/C2R + HIP k-space multiply); differentiable w.r.t. ``image``.

    Same contract as jolideco/utils/torch.py:347-370.
    """
    from ..ops import ConvPlan, ConvSameFunction, require_hip_tensor

    image_c = require_hip_tensor(image, "image")
    kernel_c = require_hip_tensor(kernel, "kernel")
    if image_c.numel() != image_c.shape[-2] * image_c.shape[-1]:
        raise NotImplementedError("only single 2-D images (1, 1, H, W) are supported")
    H, W = image_c.shape[-2:]
    kh, kw = kernel_c.shape[-2:]
    plan = ConvPlan.get(H, W, kh, kw, image_c.device)
    khat = plan.psf_spectrum(kernel_c.reshape(kh, kw))
    return ConvSameFunction.apply(image_c, None, khat, plan)


def cycle_spin_shifts(patch_shape, generator):
    """Draw the cycle-spin shifts exactly like jolideco/utils/torch.py:108-116: two `randint`
    draws from a HOST generator in [-p//4, p//4]; the first rolls rows (dim -2), the second
    columns (dim -1).  Drawing on the host keeps runs comparable with the reference CPU path and
    avoids the device->host sync of `int(shift)` in the reference."""
    wy, wx = patch_shape[0] // 4, patch_shape[1] // 4
    first = torch.randint(-wy, wy + 1, (1,), generator=generator)
    second = torch.randint(-wx, wx + 1, (1,), generator=generator)
    return int(first), int(second)


def cycle_spin_shifts_many(patch_shape, generator, n):
    """`n` consecutive draws of `cycle_spin_shifts`, in one `randint` call where both directions share a range (square
    patches): the CPU generator hands out one number per element in order, so `randint(size=(2 n,))` returns the numbers of
    2 n single draws and leaves the generator in the same state (tests/test_host_logic.py holds torch to that)."""
    wy, wx = patch_shape[0] // 4, patch_shape[1] // 4
    if wy != wx or n > 4096:
        return [cycle_spin_shifts(patch_shape, generator) for _ in range(n)]
    values = torch.randint(-wy, wy + 1, (2 * n,), generator=generator).tolist()
    return [(values[2 * i], values[2 * i + 1]) for i in range(n)]


def subpixel_offsets(generator):
    """The offsets (x0, y0) of one sub-pixel cycle spin, drawn exactly like jolideco/utils/torch.py:139-140: two float32
    `rand(1) - 0.5` draws from a HOST generator, x first.  Returned as Python floats (exact images of the float32 values)."""
    x0 = torch.rand(1, generator=generator) - 0.5
    y0 = torch.rand(1, generator=generator) - 0.5
    return float(x0), float(y0)


def subpixel_offsets_many(generator, n):
    """`n` consecutive draws of `subpixel_offsets` in one `rand` call: the CPU generator hands out one float32 per element
    in order, so `rand(2 n)` returns the numbers of 2 n single draws and leaves the generator in the same state
    (tests/test_priors_golden.py holds torch to that, for every size up to the limit used here)."""
    if n < 1 or 2 * n > SUBPIX_BATCH_MAX:
        return [subpixel_offsets(generator) for _ in range(n)]
    values = (torch.rand(2 * n, generator=generator) - 0.5).tolist()
    return [(values[2 * i], values[2 * i + 1]) for i in range(n)]


SUBPIX_BATCH_MAX = 1024  # numbers per `rand` call (an epoch of 511 datasets); more are drawn pair by pair


def subpixel_kernel(x0, y0):
    """(3, 3) float32 stencil of `grid_weights` (jolideco/utils/torch.py:31-38) for the offsets (x0, y0):
    k[i][j] = wx(j - 1) wy(i - 1), w(t) = 1 - |t - o| where |t - o| < 1, else 0, in float32 operations."""
    grid = torch.arange(-1, 2)
    y, x = torch.meshgrid(grid, grid, indexing="ij")
    x0, y0 = torch.tensor([x0], dtype=torch.float32), torch.tensor([y0], dtype=torch.float32)
    dx = torch.abs(x - x0)
    dx = torch.where(dx < 1, 1 - dx, 0)
    dy = torch.abs(y - y0)
    dy = torch.where(dy < 1, 1 - dy, 0)
    return dx * dy


def _jitter_axis(n, patch, stride):
    """(base positions, safe) along one axis of length n: ``arange(overlap, n - stride - overlap, stride)``, and whether the
    largest draw keeps the last patch inside, ``max(base) + overlap <= n - patch``."""
    overlap = patch - stride
    base = list(range(overlap, n - stride - overlap, stride))
    return base, bool(base) and base[-1] + overlap <= n - patch


def jitter_stride_check(patch, stride):
    """``int(stride)`` where a jittered patch grid of ``patch`` x ``patch`` patches can be safe at it: in [patch / 2, patch].
    ValueError otherwise -- outside [1, patch] there is no grid, and below half a patch a draw of +overlap pushes the last
    patch of EVERY image height and width outside (the reference's own jitter test, stride 3 on 37 x 37, is such a case)."""
    patch, stride = int(patch), int(stride)
    if not 1 <= stride <= patch:
        raise ValueError(f"a jittered patch grid needs a stride in [1, {patch}], got {stride}")
    if 2 * stride < patch:
        raise ValueError(
            f"a jittered patch grid of {patch} x {patch} patches at stride {stride}: no image height or width is safe at this "
            f"stride -- with overlap {patch - stride} > stride a draw can push the last patch of any axis outside the image; "
            f"the stride must be at least {(patch + 1) // 2} (half a patch)"
        )
    return stride


def jitter_grid(shape, patch_shape, stride):
    """Base positions ``(base_y, base_x)`` (int64 tensors) of the jittered patch grid of an image of ``shape`` --
    jolideco/utils/torch.py:299-302: ``arange(overlap, n - stride - overlap, stride)`` with ``overlap = patch - stride``; patch
    (i, j) is cut at ``(base_y[i] + jitter_y[i], base_x[j] + jitter_x[j])`` with draws in [-overlap, overlap].

    The reference keeps nothing inside the image and fails with an IndexError on an unlucky draw.  Here a shape is refused
    up front with a ValueError unless it has a patch along both axes and NO draw can push one outside:
    ``max(base) + overlap <= n - patch`` (for the default stride of half a patch: n a multiple of the stride).  A safe axis
    has ``overlap <= stride`` -- the last base position L obeys ``L + stride >= n - stride - overlap`` and
    ``L + overlap <= n - patch`` -- so below half a patch NO length is safe, and such a stride is refused whatever the shape
    (`jitter_stride_check`); from half a patch on, ``n = L + overlap + patch`` is safe for every L of the grid (at overlap 0
    the ``arange`` stops short of it: every n > patch is safe)."""
    patch = max(patch_shape)
    stride = jitter_stride_check(patch, stride)
    bases = []
    for axis, n in (("height", int(shape[-2])), ("width", int(shape[-1]))):
        base, safe = _jitter_axis(n, patch, stride)
        if not safe:
            below = next((m for m in range(n - 1, 0, -1) if _jitter_axis(m, patch, stride)[1]), None)
            # (2 stride >= patch: a safe length exists within a stride above n, or is the smallest one, at most 3 patches)
            above = next((m for m in range(n + 1, n + 4 * patch + 2) if _jitter_axis(m, patch, stride)[1]), None)
            what = "has no jittered patch" if not base else "lets a draw push a patch outside the image"
            near = " or ".join(str(m) for m in (below, above) if m is not None) or "not within four patches"
            raise ValueError(
                f"the {axis} {n} of an image of shape {tuple(int(v) for v in shape[-2:])} {what} at patch size {patch} and "
                f"stride {stride}: the nearest safe {axis} is {near}"
            )
        bases.append(torch.tensor(base, dtype=torch.int64))
    return bases[0], bases[1]


def jitter_draws(generator, n_x, n_y, overlap):
    """The draws of one jittered evaluation exactly like jolideco/utils/torch.py:304-318: two `randint` calls in
    [-overlap, overlap] from a HOST generator, ``(n_x,)`` FIRST, then ``(n_y,)`` -- both made when ``overlap == 0`` too
    (the generator advances).  Returns ``(jitter_x, jitter_y)``, int64 tensors."""
    jitter_x = torch.randint(low=-overlap, high=overlap + 1, size=(n_x,), generator=generator)
    jitter_y = torch.randint(low=-overlap, high=overlap + 1, size=(n_y,), generator=generator)
    return jitter_x, jitter_y


def cycle_spin(image, patch_shape, generator):
    """Rolled copy of ``image`` (jolideco/utils/torch.py:91-119).  The accelerated prior never
    materialises this: the roll is folded into the kernel's addressing."""
    shifts = cycle_spin_shifts(patch_shape, generator)
    return torch.roll(image, shifts=shifts, dims=(image.ndim - 2, image.ndim - 1))


def get_default_generator(device="cpu"):
    """Host generator with torch's default seed (jolideco/utils/torch.py:393-414).  The shifts
    are always drawn on the host, so the device argument is accepted and ignored."""
    return torch.Generator(device="cpu")


def view_as_overlapping_patches_torch(image, shape, stride=None):
    """(n_patches, p*p) view of overlapping patches (jolideco/utils/torch.py:251-275); a torch
    view helper for inspection -- the prior kernel builds patches in registers instead."""
    if stride is None:
        stride = shape[0] // 2
    win = image.unfold(image.ndim - 2, shape[0], stride).unfold(image.ndim - 1, shape[0], stride)
    return win.reshape(-1, shape[0] * shape[1])

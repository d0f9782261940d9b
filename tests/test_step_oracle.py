"""CPU: tests/step_oracle.py (the explicit float64 statement the step-kernel tests compare with) against the project's
oracle `oracle.cpu_ref` (grid_sample shift, rfft2 convolution, avg_pool2d, F.poisson_nll_loss) in float64."""
import numpy as np
import pytest
import torch

import step_oracle
from oracle import cpu_ref


def _inputs(Hd, Wd, k, U, seed):
    rs = np.random.RandomState(seed)
    psf = 0.2 + rs.uniform(size=(U * k, U * k)) ** 3
    return {
        "flux": 0.5 + rs.gamma(2.0, size=(U * Hd, U * Wd)),
        "exposure": rs.uniform(0.5, 1.5, size=(U * Hd, U * Wd)),
        "psf": psf / psf.sum(),
        "background": rs.uniform(0.5, 1.0, size=(Hd, Wd)),
        "counts": rs.poisson(6.0, size=(Hd, Wd)).astype(np.float64),
    }


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("shift", [(0.3, -0.2), (-1.6, 2.25), (-5.6, 4.4)])
@pytest.mark.parametrize("scale", [1, 2])
def test_explicit_shift_matches_grid_sample(shift, scale):
    """`shift_explicit` against `cpu_ref.shift_image` (affine_grid + grid_sample) in float64, non-integer shifts up to
    (-5.6, 4.4) x 2 pixels: same values to 1e-12 of the maximum, exact zeros where the window has left the image."""
    rs = np.random.RandomState(3)
    image = 0.5 + rs.gamma(2.0, size=(23, 31))
    with cpu_ref.precision(np.float64):
        ref = cpu_ref.shift_image(cpu_ref._tensor(image)[None, None], torch.tensor([list(shift)]), scale=scale)[0, 0].numpy()
    got = step_oracle.shift_explicit(torch.tensor(image), scale * torch.tensor(shift, dtype=torch.float64)).numpy()
    assert _rel(got, ref) < 1e-12
    assert np.array_equal(got == 0, ref == 0)
    sx, sy = scale * shift[0], scale * shift[1]
    gone = np.zeros(image.shape, dtype=bool)  # both source rows / columns of the window outside the image
    rows, cols = np.arange(23)[:, None] + np.floor(sy), np.arange(31)[None, :] + np.floor(sx)
    gone |= (rows + 1 < 0) | (rows > 22) | (cols + 1 < 0) | (cols > 30)
    assert np.all(got[gone] == 0) and (gone.any() or max(abs(sx), abs(sy)) < 1)


@pytest.mark.parametrize("U", [1, 2, 3])
@pytest.mark.parametrize("conv", ["direct", "fft"])
def test_step_oracle_matches_cpu_ref(U, conv):
    """Loss, d / d flux, d / d shift and d / d log norm of `step_oracle` against autograd of `cpu_ref.DatasetRef.loss` under
    `cpu_ref.precision(np.float64)`: non-integer shifts, even and odd PSF sizes, agreement at 1e-12 relative."""
    for seed, (Hd, Wd, k), shift, norm in ((1, (13, 18, 5), (0.3, -0.2), 1.1), (2, (12, 17, 4), (-1.6, 2.25), 0.8),
                                           (3, (16, 14, 3), (3.01, -2.4), 1.3)):
        d = _inputs(Hd, Wd, k, U, seed)
        got = step_oracle.step_oracle(d["flux"], d["exposure"], d["psf"], d["background"], d["counts"], U, shift=shift,
                                      log_norm=np.log(norm), conv=conv)
        assert step_oracle.clip_margin(got["pooled"]) >= 1e-3
        with cpu_ref.precision(np.float64):
            t = lambda a: cpu_ref._tensor(a)[None, None]  # noqa: E731
            cal = cpu_ref.CalibrationRef.create(shift[0], shift[1], norm)
            ref = cpu_ref.DatasetRef(counts=t(d["counts"]), background=t(d["background"]), exposures=[t(d["exposure"])],
                                     psfs=[t(d["psf"])], upsampling_factors=[U], calibration=cal)
            flux = t(d["flux"]).requires_grad_(True)
            loss = ref.loss((flux,))
            loss.backward()
        assert abs(got["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        assert _rel(got["grad_flux"], flux.grad.numpy()[0, 0]) < 1e-12
        assert _rel(got["grad_shift"], cal.shift_xy.grad.numpy().ravel()) < 1e-12
        assert abs(got["grad_log_norm"] - float(cal.log_background_norm.grad)) <= 1e-12 * abs(float(cal.log_background_norm.grad))


def test_step_oracle_uncalibrated_and_two_components():
    """Without a calibration the oracle is `cpu_ref.npred_total` + `poisson_nll`; two components add their clipped terms."""
    U = 2
    a, b = _inputs(10, 12, 3, U, 4), _inputs(10, 12, 3, U, 5)
    got = step_oracle.step_oracle([a["flux"], b["flux"]], [a["exposure"], b["exposure"]], [a["psf"], b["psf"]], a["background"],
                                  a["counts"], U)
    assert got["grad_shift"] is None and got["grad_log_norm"] is None
    with cpu_ref.precision(np.float64):
        t = lambda x: cpu_ref._tensor(x)[None, None]  # noqa: E731
        fluxes = [t(a["flux"]).requires_grad_(True), t(b["flux"]).requires_grad_(True)]
        npred = cpu_ref.npred_total(fluxes, [t(a["exposure"]), t(b["exposure"])], [t(a["psf"]), t(b["psf"])], t(a["background"]), [U, U])
        loss = cpu_ref.poisson_nll(npred, t(a["counts"]))
        loss.backward()
    assert abs(got["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    for g, f in zip(got["grad_flux"], fluxes):
        assert _rel(g, f.grad.numpy()[0, 0]) < 1e-12


def test_integer_shift_takes_the_right_hand_derivative():
    """At an exactly integer shift the weights are 0 and 1 and d / d shift is the slope towards the NEXT pixel."""
    image = torch.tensor(np.arange(20.0).reshape(4, 5) ** 2)
    s = torch.tensor([1.0, -1.0], dtype=torch.float64, requires_grad=True)
    out = step_oracle.shift_explicit(image, s)
    assert torch.equal(out.detach(), step_oracle.translate(image, -1, 1))
    out[1, 1].backward()  # = image[0, 2] at the shift; d/dx -> image[0, 3] - image[0, 2], d/dy -> image[1, 2] - image[0, 2]
    assert s.grad.tolist() == [float(image[0, 3] - image[0, 2]), float(image[1, 2] - image[0, 2])]

"""CPU: the oracle of tests/optimizer_cases.py (torch.optim.Adam / SGD through the reference's flux parameterisation)
pinned with answers known in closed form, and its float32 error against float64 -- the figure that sets the bound of
tests/test_gpu_optimizer_step.py."""
import numpy as np
import pytest
import torch

import optimizer_cases as cases

N = 4099
MODES = [(False, False), (False, True), (True, False), (True, True)]  # (sgd, linear)
MODE_IDS = ["adam-log", "adam-linear", "sgd-log", "sgd-linear"]


def dflux_dtheta(theta0, mask, linear):
    d = np.ones_like(theta0, dtype=np.float64) if linear else np.exp(theta0.astype(np.float64))
    return d if mask is None else d * mask


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("linear", [False, True], ids=["log", "linear"])
@pytest.mark.parametrize("hyper", sorted(cases.HYPER))
def test_first_adam_step_from_zero_moments_is_lr_g_over_abs_g_plus_eps(hyper, linear, masked):
    """m = (1 - b1) g, v = (1 - b2) g^2 and both bias corrections cancel: theta1 = theta0 - lr g / (|g| + eps)."""
    lr, betas, eps = cases.HYPER[hyper]
    theta0, mask, grads, _ = cases.draw_case(N, 1, masked=masked)
    out = cases.oracle(theta0, mask, grads, linear=linear, sgd=False, lr=lr, betas=betas, eps=eps, dtype=torch.float64)
    g = grads[0].astype(np.float64) * dflux_dtheta(theta0, mask, linear)
    want = theta0.astype(np.float64) - lr * g / (np.abs(g) + eps)
    assert np.max(np.abs(out["theta"][0] - want)) <= 1e-12
    np.testing.assert_allclose(out["exp_avg"][0], (1 - betas[0]) * g, rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["exp_avg_sq"][0], (1 - betas[1]) * g * g, rtol=1e-12, atol=0)
    want_flux = want if linear else np.exp(want)
    np.testing.assert_allclose(out["flux"][0], want_flux if mask is None else want_flux * mask, rtol=1e-12, atol=0)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("linear", [False, True], ids=["log", "linear"])
def test_sgd_step_is_theta_minus_lr_g(linear, masked):
    lr = cases.learning_rate(0.1, True, linear)
    theta0, mask, grads, _ = cases.draw_case(N, 1, masked=masked)
    out = cases.oracle(theta0, mask, grads, linear=linear, sgd=True, lr=lr, dtype=torch.float64)
    g = grads[0].astype(np.float64) * dflux_dtheta(theta0, mask, linear)
    assert np.max(np.abs(out["theta"][0] - (theta0.astype(np.float64) - lr * g))) <= 1e-12
    assert sorted(out) == ["flux", "theta"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("sgd,linear", MODES, ids=MODE_IDS)
def test_masked_and_zero_gradient_pixels_do_not_move(sgd, linear, dtype):
    """A masked pixel has flux 0 and gradient 0 in every step, so its moments stay 0 and theta stays where it was, bit
    for bit; so does an unmasked pixel whose flux gradient is exactly zero in every step."""
    theta0, mask, grads, zero_always = cases.draw_case(N, 5, masked=True)
    out = cases.oracle(theta0, mask, grads, linear=linear, sgd=sgd, lr=cases.learning_rate(0.1, sgd, linear), dtype=dtype)
    start = theta0.astype(out["theta"][0].dtype)
    off = mask == 0
    assert 0.1 < off.mean() < 0.3 and len(zero_always) >= 2
    for step in range(5):
        assert np.array_equal(out["theta"][step][off], start[off])
        assert np.all(out["flux"][step][off] == 0)
        assert np.array_equal(out["theta"][step][zero_always], start[zero_always])
        if not sgd:
            assert np.all(out["exp_avg"][step][off] == 0) and np.all(out["exp_avg_sq"][step][off] == 0)
    moved = (out["theta"][-1] != start)
    assert moved[~off].mean() > 0.95


@pytest.mark.parametrize("sgd,linear", MODES, ids=MODE_IDS)
def test_a_run_started_from_state_and_step_count_is_the_tail_of_the_longer_run(sgd, linear):
    """exp_avg0, exp_avg_sq0 and step0 go in through the optimizer's state: 2 + 3 steps equal 5 steps exactly."""
    theta0, mask, grads, _ = cases.draw_case(N, 5, masked=True)
    kw = dict(linear=linear, sgd=sgd, lr=cases.learning_rate(0.1, sgd, linear), dtype=torch.float64)
    whole = cases.oracle(theta0, mask, grads, **kw)
    state = {} if sgd else {"exp_avg0": whole["exp_avg"][1], "exp_avg_sq0": whole["exp_avg_sq"][1], "step0": 2}
    tail = cases.oracle(whole["theta"][1], mask, grads[2:], **state, **kw)
    for key in whole:
        for step in range(3):
            assert np.array_equal(tail[key][step], whole[key][2 + step]), (key, step)
    if not sgd:  # the step count matters: the same moments under another count give another theta
        other = cases.oracle(whole["theta"][1], mask, grads[2:], **{**state, "step0": 0}, **kw)
        assert not np.array_equal(other["theta"][0], whole["theta"][2])


def test_flux_rel_error_is_per_pixel_and_skips_masked_pixels():
    want = np.array([1e-6, 1.0, 100.0, 5.0])
    got = want + np.array([1e-9, 1e-6, 1e-6, 3.0])
    mask = np.array([1.0, 1.0, 1.0, 0.0])
    assert cases.flux_rel_error(got, want, mask) == pytest.approx(1e-3)
    assert cases.flux_rel_error(got, want) == pytest.approx(0.6)
    assert cases.rel_linf(got[:3], want[:3]) < 2e-8  # (what the max-normalised measure makes of the faint pixel)
    assert cases.bound(1e-9) == 1e-6 and cases.bound(1e-6) == 4e-6


@pytest.mark.parametrize("sgd,linear", MODES, ids=MODE_IDS)
def test_float32_oracle_error_on_theta_leaves_the_floor_as_the_bound(sgd, linear):
    """The float32 oracle against the float64 one after 5 steps at n = 4099, masked: printed for every quantity, and
    below 2.5e-7 on theta, so that bound() of it is the 1e-6 floor."""
    theta0, mask, grads, _ = cases.draw_case(N, 5, masked=True)
    kw = dict(linear=linear, sgd=sgd, lr=cases.learning_rate(0.1, sgd, linear))
    ref64 = cases.oracle(theta0, mask, grads, dtype=torch.float64, **kw)
    ref32 = cases.oracle(theta0, mask, grads, dtype=torch.float32, **kw)
    assert ref32["theta"][0].dtype == np.float32 and ref64["theta"][0].dtype == np.float64
    own = cases.errors(ref32, ref64, mask, 4)
    print(f"float32 oracle, sgd={sgd} linear={linear}: " + ", ".join(f"{k} {v:.2e}" for k, v in own.items()))
    assert 0 < own["theta"] < 2.5e-7
    assert cases.bound(own["theta"]) == 1e-6

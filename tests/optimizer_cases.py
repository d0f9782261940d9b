"""Shared by tests/test_optimizer_oracle.py (CPU) and tests/test_gpu_optimizer_step.py (GPU): the seeded inputs of the
optimizer step tests and their oracle, `torch.optim.Adam` / `torch.optim.SGD` themselves on the CPU in float64 / float32,
driven through the reference's parameterisation of a flux component (jolideco/models/core.py:584-594): theta is the
parameter, flux = exp(theta) (log flux) or theta (linear), times the mask; every step is `flux.backward(grad_flux)` and
`opt.step()`.  Nothing here restates the update of csrc/jd_adam.h."""
import functools

import numpy as np
import torch

from prior_cases import bound, rel_linf  # noqa: F401  (the project's rule, re-exported for the two test modules)

# (lr, betas, eps): torch.optim.Adam's defaults at the fits' learning rate, and a set where every term differs
HYPER = {"default": (0.1, (0.9, 0.999), 1e-8), "other": (0.02, (0.8, 0.95), 1e-5)}
WARM_STEPS = 3  # a trajectory starts from the moments and the step count of this many float64 steps
# SGD on a log-flux parameter moves theta by lr * grad_flux * exp(theta) in one step.  With the gradients of `draw_case`
# (|grad_flux| up to 4 sigma * 10^2, exp(theta) up to e^4: |g| up to 2e4) a learning rate of 0.1 moves theta by up to
# 2000 -- exp overflows float32 (> 88.7) after the first step, the float32 oracle ends in inf / nan and has no error
# against float64 to speak of.  Adam's steps are bounded by lr whatever the gradient, and linear SGD by lr * 4e2, so only
# log-flux SGD takes its learning rate times this factor: steps of at most 0.2, theta within [-6, 6] over a trajectory.
SGD_LOG_LR_SCALE = 1e-4


def learning_rate(lr, sgd, linear):
    return lr * SGD_LOG_LR_SCALE if sgd and not linear else lr


def draw_case(n, n_steps, seed=0, masked=True):
    """theta0 ~ N(0, 1), `n_steps` gradients ~ N(0, 1) * 10**U(-3, 2) per pixel (sqrt(v) from eps-dominated to large) with
    a handful of exact zeros, and a 0 / 1 mask with about 20 % zeros (None: no mask) -- float32, so that the oracle in
    either precision and the kernels read the same numbers."""
    rs = np.random.RandomState(9000 + 17 * seed + n % 9973)
    theta0 = rs.normal(size=n).astype(np.float32)
    n_zero = 1 if n < 16 else 3
    grads = []
    for _ in range(n_steps):
        g = (rs.normal(size=n) * 10.0 ** rs.uniform(-3, 2, size=n)).astype(np.float32)
        g[rs.choice(n, size=n_zero, replace=False)] = 0.0
        grads.append(g)
    zero_always = rs.choice(n, size=n_zero, replace=False)  # pixels whose gradient is zero in EVERY step
    for g in grads:
        g[zero_always] = 0.0
    mask = None
    if masked:
        mask = (rs.uniform(size=n) >= 0.2).astype(np.float32)
        mask[0], mask[n - 1] = 0.0, 1.0  # (both kinds at every size; n >= 2)
    return theta0, mask, grads, zero_always


def to_flux(theta, mask, linear):
    flux = theta if linear else torch.exp(theta)
    return flux if mask is None else flux * mask


def oracle(theta0, mask, grads, *, linear, sgd, lr, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64, exp_avg0=None,
           exp_avg_sq0=None, step0=0):
    """Steps of torch.optim on theta with the gradients `grads` of the loss with respect to the FLUX.  Returns a dict of
    lists with one numpy array per step: "theta", "flux" (of the new theta) and, Adam only, "exp_avg" / "exp_avg_sq".
    `exp_avg0`, `exp_avg_sq0`, `step0`: the optimizer's state before the first step (a run that starts mid-trajectory)."""
    as_t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype).clone()  # noqa: E731
    theta = torch.nn.Parameter(as_t(theta0))
    mask_t = None if mask is None else as_t(mask)
    if sgd:
        opt = torch.optim.SGD([theta], lr=lr)
    else:
        opt = torch.optim.Adam([theta], lr=lr, betas=betas, eps=eps, foreach=False)
        if step0 or exp_avg0 is not None or exp_avg_sq0 is not None:
            zeros = np.zeros(theta.shape)
            opt.state[theta] = {"step": torch.tensor(float(step0)),
                                "exp_avg": as_t(zeros if exp_avg0 is None else exp_avg0),
                                "exp_avg_sq": as_t(zeros if exp_avg_sq0 is None else exp_avg_sq0)}
    out = {"theta": [], "flux": []} if sgd else {"theta": [], "flux": [], "exp_avg": [], "exp_avg_sq": []}
    for g in grads:
        opt.zero_grad()
        to_flux(theta, mask_t, linear).backward(as_t(g))
        opt.step()
        with torch.no_grad():
            out["theta"].append(theta.detach().numpy().copy())
            out["flux"].append(to_flux(theta, mask_t, linear).numpy().copy())
        if not sgd:
            out["exp_avg"].append(opt.state[theta]["exp_avg"].numpy().copy())
            out["exp_avg_sq"].append(opt.state[theta]["exp_avg_sq"].numpy().copy())
    return out


def flux_rel_error(got, want, mask=None):
    """Largest error of a flux pixel relative to ITS OWN value, over the unmasked pixels (a measure normalised by the
    brightest pixel would hide the faint ones)."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    keep = np.ones(want.shape, dtype=bool) if mask is None else np.asarray(mask).ravel() != 0
    keep &= want != 0
    return float(np.max(np.abs(got - want)[keep] / np.abs(want)[keep]))


QUANTITIES = {"theta": rel_linf, "exp_avg": rel_linf, "exp_avg_sq": rel_linf}


def errors(got, want, mask, step):
    """{quantity: error} of step `step` of `got` against `want` (both as `oracle` returns them): theta and the moments by
    relative L-inf, the flux by `flux_rel_error`."""
    out = {key: fn(got[key][step], want[key][step]) for key, fn in QUANTITIES.items() if key in want}
    out["flux"] = flux_rel_error(got["flux"][step], want["flux"][step], mask)
    return out


@functools.lru_cache(maxsize=3)  # (the tests ask for a trajectory in runs of cases; the largest holds some 0.5 GB)
def trajectory(n, masked, linear, sgd, hyper="default", n_steps=4, seed=0):
    """A run that starts mid-trajectory, computed once and shared: WARM_STEPS float64 steps from zero moments, their
    theta and moments rounded to float32 as the start (Adam: step count WARM_STEPS), then `n_steps` steps with fresh
    gradients by the float64 and by the float32 oracle.  Returns a dict: "theta0", "exp_avg0", "exp_avg_sq0" (float32; the
    moments None with SGD), "mask", "grads", "step0", "ref64", "ref32" and "hyper" = (lr, betas, eps)."""
    lr, betas, eps = HYPER[hyper]
    lr = learning_rate(lr, sgd, linear)
    theta0, mask, grads, _ = draw_case(n, WARM_STEPS + n_steps, seed=seed, masked=masked)
    kw = dict(linear=linear, sgd=sgd, lr=lr, betas=betas, eps=eps)
    warm = oracle(theta0, mask, grads[:WARM_STEPS], dtype=torch.float64, **kw)
    start = {"theta0": warm["theta"][-1].astype(np.float32), "exp_avg0": None, "exp_avg_sq0": None}
    if not sgd:
        start["exp_avg0"] = warm["exp_avg"][-1].astype(np.float32)
        start["exp_avg_sq0"] = warm["exp_avg_sq"][-1].astype(np.float32)
    step0 = 0 if sgd else WARM_STEPS
    refs = {name: oracle(start["theta0"], mask, grads[WARM_STEPS:], dtype=dtype, exp_avg0=start["exp_avg0"],
                         exp_avg_sq0=start["exp_avg_sq0"], step0=step0, **kw)
            for name, dtype in (("ref64", torch.float64), ("ref32", torch.float32))}
    return {**start, "mask": mask, "grads": grads[WARM_STEPS:], "step0": step0, "hyper": (lr, betas, eps), **refs}

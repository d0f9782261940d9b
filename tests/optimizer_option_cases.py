"""Shared by tests/test_optimizer_options_oracle.py (CPU) and tests/test_gpu_optimizer_options.py (GPU): the option sets
of the optimizer step with torch.optim's options, seeded inputs as in tests/optimizer_cases.py (`draw_case`), and the
oracle -- `torch.optim.Adam` / `torch.optim.SGD` themselves WITH the option kwargs, on the CPU in float64 / float32,
through theta -> flux -> `backward(grad_flux)`.  Nothing here restates an update of csrc/optimizer.hip."""
import functools

import numpy as np
import torch

import optimizer_cases as plain
from optimizer_cases import bound, flux_rel_error, rel_linf, to_flux  # noqa: F401  (re-exported for the two test modules)

LR = 0.1
BETAS, EPS = (0.9, 0.999), 1e-8
WARM_STEPS = plain.WARM_STEPS
N_STEPS = 4
# name -> (sgd, kwargs of torch.optim)
OPTION_SETS = {
    "adam-wd": (False, {"weight_decay": 0.05}),
    "adam-amsgrad": (False, {"amsgrad": True}),
    "adam-wd-amsgrad": (False, {"weight_decay": 0.05, "amsgrad": True}),
    "adam-wd-decoupled": (False, {"weight_decay": 0.05, "decoupled_weight_decay": True}),
    "adam-wd-decoupled-amsgrad": (False, {"weight_decay": 0.05, "decoupled_weight_decay": True, "amsgrad": True}),
    "sgd-momentum": (True, {"momentum": 0.9}),
    "sgd-momentum-dampening": (True, {"momentum": 0.9, "dampening": 0.25}),
    "sgd-momentum-nesterov": (True, {"momentum": 0.9, "nesterov": True}),
    "sgd-wd": (True, {"weight_decay": 0.05}),
    "sgd-momentum-wd-nesterov": (True, {"momentum": 0.9, "weight_decay": 0.05, "nesterov": True}),
}
STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "momentum_buffer")


def learning_rate(sgd, linear, options):
    """`optimizer_cases.learning_rate`, and for log-flux SGD times (1 - momentum): a momentum of 0.9 sums steps of one
    sign to ten times a single step, and exp(theta) must stay inside float32 over the trajectory."""
    lr = plain.learning_rate(LR, sgd, linear)
    return lr * (1.0 - options.get("momentum", 0.0)) if sgd and not linear else lr


def oracle(theta0, mask, grads, *, linear, sgd, lr, options, dtype=torch.float64, state0=None, step0=0):
    """Steps of torch.optim with the kwargs ``options`` on theta, with the gradients `grads` of the loss with respect to the
    FLUX.  Returns a dict of lists, one numpy array per step: "theta", "flux" (of the new theta) and every state image the
    optimizer keeps (`STATE_KEYS`).  ``state0`` / ``step0``: Adam's state before the first step (a run that starts
    mid-trajectory); SGD always starts without a momentum buffer, so that its first step is the special one."""
    as_t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype).clone()  # noqa: E731
    theta = torch.nn.Parameter(as_t(theta0))
    mask_t = None if mask is None else as_t(mask)
    if sgd:
        opt = torch.optim.SGD([theta], lr=lr, **options)
    else:
        opt = torch.optim.Adam([theta], lr=lr, betas=BETAS, eps=EPS, foreach=False, **options)
        if state0 is not None:
            opt.state[theta] = {"step": torch.tensor(float(step0)), **{key: as_t(value) for key, value in state0.items()}}
    out = {"theta": [], "flux": []}
    for g in grads:
        opt.zero_grad()
        to_flux(theta, mask_t, linear).backward(as_t(g))
        opt.step()
        with torch.no_grad():
            out["theta"].append(theta.detach().numpy().copy())
            out["flux"].append(to_flux(theta, mask_t, linear).numpy().copy())
        for key in STATE_KEYS:
            value = opt.state[theta].get(key)
            if value is not None:
                out.setdefault(key, []).append(value.detach().numpy().copy())
    return out


def errors(got, want, mask, step):
    """{quantity: error} of step `step`: theta and every state image by relative L-inf, the flux per pixel."""
    out = {key: rel_linf(got[key][step], want[key][step]) for key in ("theta",) + STATE_KEYS if key in want}
    out["flux"] = flux_rel_error(got["flux"][step], want["flux"][step], mask)
    return out


@functools.lru_cache(maxsize=4)
def trajectory(name, n, masked, linear, n_steps=N_STEPS, seed=0):
    """The run of option set ``name``, computed once and shared.  Adam starts mid-trajectory: WARM_STEPS float64 steps from
    zero state, theta and every state image (max_exp_avg_sq included) rounded to float32 as the start, step count
    WARM_STEPS.  SGD starts from step 0.  Then `n_steps` steps with fresh gradients by the float64 and the float32 oracle.
    Returns a dict: "theta0", "state0" ({} for SGD), "mask", "grads", "step0", "lr", "options", "sgd", "ref64", "ref32"."""
    sgd, options = OPTION_SETS[name]
    lr = learning_rate(sgd, linear, options)
    warm_steps = 0 if sgd else WARM_STEPS
    theta0, mask, grads, _ = plain.draw_case(n, warm_steps + n_steps, seed=seed, masked=masked)
    kw = dict(linear=linear, sgd=sgd, lr=lr, options=options)
    state0 = {}
    if not sgd:
        warm = oracle(theta0, mask, grads[:warm_steps], dtype=torch.float64, **kw)
        theta0 = warm["theta"][-1].astype(np.float32)
        state0 = {key: warm[key][-1].astype(np.float32) for key in STATE_KEYS if key in warm}
    refs = {ref: oracle(theta0, mask, grads[warm_steps:], dtype=dtype, state0=state0 or None, step0=warm_steps, **kw)
            for ref, dtype in (("ref64", torch.float64), ("ref32", torch.float32))}
    return {"theta0": theta0, "state0": state0, "mask": mask, "grads": grads[warm_steps:], "step0": warm_steps, "lr": lr,
            "options": options, "sgd": sgd, **refs}

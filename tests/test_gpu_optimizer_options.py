"""GPU: the optimizer step with torch.optim's options (csrc/optimizer.hip: jd_optimizer_step, jd_optimizer_step_multi).

A  the step against torch.optim WITH the option kwargs in float64 (tests/optimizer_option_cases.py): every option set, log
   and linear flux, with and without mask, the float4 and the scalar kernel, the second trip of both grid-stride loops;
   theta, every state image and the flux after every step under bound() of the float32 oracle's own error.
B  variants that must give the same bits: unaligned images (scalar kernel), the device-resident bias terms,
   jd_optimizer_step_multi against per-tensor calls, and -- every option off -- jd_adam_step / jd_sgd_step.
C  sessions: option keys at their defaults change no bit of a fit; an Adam-option fit replayed from captured epochs equals
   its by-value epochs.
D  two fits against the live reference (tests/golden/optimizer_options.npz, tools/make_golden_optimizer_options.py).

Largest figures of part A on an MI355X, per option set and flux form over every size and mask (kernel | float32 oracle of the
step at which the kernel's figure is largest, both against float64):
  adam-amsgrad log                 : theta 1.02e-07 | 1.02e-07, exp_avg 9.46e-08 | 9.46e-08, exp_avg_sq 2.03e-07 | 2.03e-07, max_exp_avg_sq 2.03e-07 | 2.03e-07, flux 3.68e-07 | 3.68e-07
  adam-amsgrad linear              : theta 1.17e-07 | 1.17e-07, exp_avg 1.13e-07 | 5.98e-08, exp_avg_sq 1.31e-07 | 3.39e-08, max_exp_avg_sq 8.24e-08 | 2.22e-10, flux 1.81e-04 | 7.20e-04
  adam-wd log                      : theta 9.20e-08 | 9.20e-08, exp_avg 1.90e-07 | 5.84e-08, exp_avg_sq 3.75e-07 | 2.75e-07, flux 3.10e-07 | 3.10e-07
  adam-wd linear                   : theta 8.28e-08 | 8.28e-08, exp_avg 9.94e-08 | 9.94e-08, exp_avg_sq 1.63e-07 | 9.27e-08, flux 1.68e-05 | 8.53e-05
  adam-wd-amsgrad log              : theta 9.96e-08 | 8.43e-08, exp_avg 1.43e-07 | 7.28e-08, exp_avg_sq 2.84e-07 | 1.84e-07, max_exp_avg_sq 2.84e-07 | 1.84e-07, flux 4.48e-07 | 4.48e-07
  adam-wd-amsgrad linear           : theta 9.44e-08 | 9.44e-08, exp_avg 9.27e-08 | 9.27e-08, exp_avg_sq 1.63e-07 | 9.27e-08, max_exp_avg_sq 8.47e-08 | 8.47e-08, flux 5.65e-04 | 4.56e-04
  adam-wd-decoupled log            : theta 1.32e-07 | 1.28e-07, exp_avg 2.90e-07 | 4.53e-07, exp_avg_sq 5.95e-07 | 8.85e-07, flux 4.30e-07 | 3.94e-07
  adam-wd-decoupled linear         : theta 8.96e-08 | 1.34e-07, exp_avg 1.13e-07 | 5.98e-08, exp_avg_sq 1.31e-07 | 3.39e-08, flux 1.29e-05 | 3.32e-05
  adam-wd-decoupled-amsgrad log    : theta 1.12e-07 | 1.53e-07, exp_avg 1.36e-07 | 1.11e-07, exp_avg_sq 3.05e-07 | 1.90e-07, max_exp_avg_sq 3.05e-07 | 1.90e-07, flux 3.60e-07 | 4.74e-07
  adam-wd-decoupled-amsgrad linear : theta 1.14e-07 | 1.55e-07, exp_avg 1.13e-07 | 5.98e-08, exp_avg_sq 1.31e-07 | 3.39e-08, max_exp_avg_sq 8.24e-08 | 2.22e-10, flux 7.57e-06 | 4.09e-06
  sgd-momentum log                 : theta 8.67e-08 | 8.67e-08, momentum_buffer 1.50e-07 | 1.50e-07, flux 2.88e-07 | 2.88e-07
  sgd-momentum linear              : theta 1.10e-07 | 1.10e-07, momentum_buffer 1.38e-07 | 1.38e-07, flux 1.65e-05 | 1.65e-05
  sgd-momentum-dampening log       : theta 9.33e-08 | 9.33e-08, momentum_buffer 1.51e-07 | 1.51e-07, flux 3.14e-07 | 3.14e-07
  sgd-momentum-dampening linear    : theta 1.16e-07 | 1.16e-07, momentum_buffer 1.94e-07 | 1.94e-07, flux 2.31e-05 | 2.31e-05
  sgd-momentum-nesterov log        : theta 1.01e-07 | 1.01e-07, momentum_buffer 2.55e-07 | 2.55e-07, flux 3.44e-07 | 3.44e-07
  sgd-momentum-nesterov linear     : theta 9.55e-08 | 9.55e-08, momentum_buffer 1.38e-07 | 1.38e-07, flux 1.28e-04 | 1.28e-04
  sgd-momentum-wd-nesterov log     : theta 9.25e-08 | 9.25e-08, momentum_buffer 1.67e-07 | 1.67e-07, flux 4.49e-07 | 4.49e-07
  sgd-momentum-wd-nesterov linear  : theta 9.24e-08 | 9.24e-08, momentum_buffer 1.70e-07 | 1.70e-07, flux 7.44e-05 | 7.44e-05
  sgd-wd log                       : theta 1.53e-07 | 1.53e-07, flux 3.77e-07 | 3.77e-07
  sgd-wd linear                    : theta 1.15e-07 | 1.15e-07, flux 8.59e-05 | 8.59e-05
(The per-pixel flux error of a LINEAR parameter is large in both columns where a step lands next to zero: the rounding of
the update against a flux a thousand times smaller.  Which float32 implementation is the unlucky one there is a matter of
operation order, and torch's own float32 kernels differ between two hosts in 2 % of the parameters, so the bound itself
moves from host to host.  Adam with options in adam_update's order missed it in 4 of these 128 cases -- 3.21e-04 | 3.22e-05
at adam-wd-amsgrad linear n = 3072, 1.80e-05 | 4.09e-06 at adam-wd-decoupled-amsgrad linear n = 1021, with and without
mask --, in the order of torch's float32 kernels as emulated on another host in the same four (2.50e-04, 1.80e-05); it now
computes a parameter's few operations in double and rounds what it stores once (csrc/optimizer.hip adam_update_wide):
7.68e-05 and 7.57e-06 there.  SGD with options gives torch's float32 bits, its columns are equal.)
The fits of part D: flux 6.54e-07 (Adam, sequential) and 2.32e-07 (SGD, joint) relative L-inf against the reference,
calibration parameters within 6e-08 absolute.
"""
import ctypes

import numpy as np
import pytest
import torch

import optimizer_cases as plain_cases
import optimizer_option_cases as cases
from conftest import rel_linf, unpack_datasets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SETS = sorted(cases.OPTION_SETS)
ADAM_SETS = [name for name in SETS if not cases.OPTION_SETS[name][0]]
STATE_NAMES = {"exp_avg": "m", "exp_avg_sq": "v", "max_exp_avg_sq": "vmax", "momentum_buffer": "buf"}


def held(array, offset=False):
    """`array` in a fresh device allocation, or (`offset`) as a view one float into an allocation of n + 1: 4-byte aligned."""
    if array is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).reshape(-1)
    buf = torch.empty(src.numel() + int(offset), device=DEV)
    view = buf[int(offset):]
    view.copy_(src)
    assert view.data_ptr() % 16 == (4 if offset else 0) and view.is_contiguous()
    return view


class Images:
    """The images of one step on the device as the start of a trajectory left them: flux_in = exp(theta) * mask (linear:
    theta * mask), Adam's state images, a momentum buffer of NaN (its first step must not read it)."""

    def __init__(self, tr, linear, offsets=()):
        theta0 = tr["theta0"]
        flux = theta0.astype(np.float32) if linear else np.exp(theta0.astype(np.float64)).astype(np.float32)
        if tr["mask"] is not None:
            flux = flux * tr["mask"]
        mk = lambda name, a: held(a, name in offsets)  # noqa: E731
        self.theta, self.flux_in, self.flux_out = mk("theta", theta0), mk("flux_in", flux), mk("flux_out", np.full_like(flux, NAN))
        self.grad, self.mask = mk("grad", tr["grads"][0]), mk("mask", tr["mask"])
        options, state0 = tr["options"], tr["state0"]
        self.m, self.v, self.vmax, self.buf = None, None, None, None
        if not tr["sgd"]:
            self.m, self.v = mk("m", state0["exp_avg"]), mk("v", state0["exp_avg_sq"])
            if options.get("amsgrad"):
                self.vmax = mk("vmax", state0["max_exp_avg_sq"])
        elif options.get("momentum"):
            self.buf = mk("buf", np.full_like(flux, NAN))
        self.n = self.theta.numel()

    def present(self):
        return [name for name in ("theta", "flux_in", "flux_out", "grad", "m", "v", "vmax", "buf", "mask") if getattr(self, name) is not None]

    def result(self):
        torch.cuda.synchronize()
        out = {"theta": self.theta.clone(), "flux": self.flux_out.clone()}
        out.update({key: getattr(self, name).clone() for key, name in STATE_NAMES.items() if getattr(self, name) is not None})
        return out


def options_struct(sgd, lr, options, step=1, first_step=False, by_value=True):
    """`jd_optimizer_options` of a torch.optim kwargs dict for step number `step` (Adam: the bias terms by value, or NaN)."""
    from jolideco_amd import _hip
    from jolideco_amd.ops import adam_bias_terms

    out = _hip.OptimizerOptions(kind=_hip.OPTIMIZER_SGD if sgd else _hip.OPTIMIZER_ADAM, lr=lr, first_step=int(first_step),
                                weight_decay=options.get("weight_decay", 0.0))
    if sgd:
        out.momentum, out.dampening, out.nesterov = options.get("momentum", 0.0), options.get("dampening", 0.0), int(options.get("nesterov", False))
    else:
        beta1, beta2 = cases.BETAS
        out.step_size, out.bias2_sqrt = adam_bias_terms(step, lr, beta1, beta2) if by_value else (NAN, NAN)
        out.beta1, out.beta2, out.one_minus_beta1, out.one_minus_beta2, out.eps = beta1, beta2, 1 - beta1, 1 - beta2, cases.EPS
        out.amsgrad, out.decoupled_weight_decay = int(options.get("amsgrad", False)), int(options.get("decoupled_weight_decay", False))
    return out


def bias_device(lr, step):
    from jolideco_amd.ops import adam_bias_terms

    return torch.tensor(adam_bias_terms(step, lr, *cases.BETAS), dtype=torch.float32, device=DEV)


def option_step(s, *, sgd, lr, options, linear, step, first_step, zero_grad=0, device_bias=False):
    """jd_optimizer_step on the images of `s`."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, stream_ptr

    args = options_struct(sgd, lr, options, step, first_step, by_value=not device_bias)
    bias_dev = bias_device(lr, step) if device_bias else None
    check(_hip.lib().jd_optimizer_step(ptr(s.theta), ptr(s.flux_in), ptr(s.flux_out), ptr(s.grad), ptr(s.m), ptr(s.v), ptr(s.vmax),
                                       ptr(s.buf), ptr(s.mask), s.n, ctypes.byref(args), zero_grad, int(not linear), ptr(bias_dev),
                                       stream_ptr(DEV)))
    torch.cuda.synchronize()


def assert_same_bits(got, want, label):
    assert sorted(got) == sorted(want)
    for key in want:
        assert bool(torch.isfinite(want[key]).all()), f"{label}: {key} of the comparison is not finite"
        assert torch.equal(got[key], want[key]), f"{label}: {key} differs in {int((got[key] != want[key]).sum())} of {want[key].numel()} pixels"


def assert_within_oracle_bounds(got, tr, label):
    """`got` (as cases.oracle returns it) against the float64 oracle under bound() of the float32 oracle's own error, step by
    step and quantity by quantity; prints the largest figure of each quantity beside the oracle's own."""
    worst, failures = {}, []
    assert sorted(got) == sorted(tr["ref64"])
    for step in range(len(got["theta"])):
        err, own = cases.errors(got, tr["ref64"], tr["mask"], step), cases.errors(tr["ref32"], tr["ref64"], tr["mask"], step)
        for key in err:
            if key not in worst or err[key] > worst[key][0]:
                worst[key] = (err[key], own[key])
            if not err[key] <= cases.bound(own[key]):
                failures.append(f"step {step} {key}: {err[key]:.3e} > bound({own[key]:.3e}) = {cases.bound(own[key]):.3e}")
    print(f"\n{label}: " + ", ".join(f"{key} {e:.2e} | {o:.2e}" for key, (e, o) in worst.items()))
    assert not failures, f"{label}: " + "; ".join(failures)


# ------------------------------------------------------------------------------------------------------------------
# A: the step against float64
# ------------------------------------------------------------------------------------------------------------------
SMALL_SIZES = (4, 1020, 1021)  # one thread | float4 kernel, ragged last wave | scalar kernel
WHOLE_BLOCKS = 256 * 4 * 3
SCALAR_SECOND_TRIP = (1 << 20) + 259  # 4096 blocks x 256 pixels and a rest: the scalar kernel's loop goes round
VECTOR_SECOND_TRIP = (1 << 22) + 1024  # 4096 blocks x 1024 pixels and a rest: the float4 kernel's loop goes round


def step_cases():
    out = []

    def add(name, linear, masked, n, n_steps=cases.N_STEPS):
        out.append(pytest.param(name, linear, masked, n, n_steps,
                                id=f"{name}-{'linear' if linear else 'log'}-{'mask' if masked else 'nomask'}-n{n}"))

    for name in SETS:
        for n in SMALL_SIZES + ((WHOLE_BLOCKS,) if name in ("adam-wd-amsgrad", "sgd-momentum-wd-nesterov") else ()):
            for linear in (False, True):
                for masked in (False, True):
                    add(name, linear, masked, n)
    add("adam-wd-amsgrad", False, True, SCALAR_SECOND_TRIP, 2)
    add("sgd-momentum-wd-nesterov", False, True, VECTOR_SECOND_TRIP, 2)
    return out


@pytest.mark.parametrize("name,linear,masked,n,n_steps", step_cases())
def test_step_matches_torch_optim_with_the_options_in_float64(name, linear, masked, n, n_steps):
    """jd_optimizer_step, `n_steps` steps with fresh gradients, each on the flux the step before left -- Adam from the state
    and the step count of a three-step warm-up, SGD from step 0 with `first_step` set once: theta, every state image and
    the flux after every step against the float64 oracle; masked pixels have flux exactly 0 and, without weight decay,
    keep theta bit for bit (with it torch moves them: g = 0 + weight_decay * theta)."""
    tr = cases.trajectory(name, n, masked, linear, n_steps)
    sgd, options = tr["sgd"], tr["options"]
    s = Images(tr, linear)
    start = s.theta.clone()
    got = {key: [] for key in tr["ref64"]}
    for i in range(n_steps):
        s.grad = held(tr["grads"][i])
        before = s.grad.clone()
        option_step(s, sgd=sgd, lr=tr["lr"], options=options, linear=linear, step=tr["step0"] + 1 + i, first_step=i == 0)
        assert torch.equal(s.grad.view(torch.int32), before.view(torch.int32)), "zero_grad = 0 changed the gradient image"
        res = s.result()
        assert sorted(res) == sorted(got)
        for key in got:
            got[key].append(res[key].cpu().numpy())
        if masked:
            off = s.mask == 0
            assert bool((res["flux"][off] == 0).all()), f"step {i}: flux under the mask"
            if not options.get("weight_decay"):
                assert torch.equal(res["theta"][off].view(torch.int32), start[off].view(torch.int32)), f"step {i}: a masked theta moved"
        s.flux_in, s.flux_out = s.flux_out, s.flux_in
    assert not torch.equal(s.theta, start)
    assert_within_oracle_bounds(got, tr, f"{name} {'linear' if linear else 'log'} {'mask' if masked else 'nomask'} n={n}")


@pytest.mark.parametrize("name", ["adam-wd-amsgrad", "sgd-momentum"])
def test_zero_grad_zeroes_the_gradient_image_and_changes_nothing_else(name):
    for n in (1020, 1021):
        tr = cases.trajectory(name, n, True, False)
        kw = dict(sgd=tr["sgd"], lr=tr["lr"], options=tr["options"], linear=False, step=tr["step0"] + 1, first_step=True)
        kept, zeroed = Images(tr, False), Images(tr, False)
        option_step(kept, **kw)
        option_step(zeroed, zero_grad=1, **kw)
        assert not bool(zeroed.grad.any()) and bool(kept.grad.any())
        assert_same_bits(zeroed.result(), kept.result(), f"n={n}")


# ------------------------------------------------------------------------------------------------------------------
# B: variants that must give the same bits
# ------------------------------------------------------------------------------------------------------------------
B_SIZES = (1020, 1021)


def one_step(tr, linear, offsets=(), first_step=True, **kw):
    s = Images(tr, linear, offsets=offsets)
    if not first_step:  # (a later step reads the buffer: give it numbers)
        s.buf.copy_(held(tr["grads"][1]))
    option_step(s, sgd=tr["sgd"], lr=tr["lr"], options=tr["options"], linear=linear, step=tr["step0"] + 1, first_step=first_step, **kw)
    return s.result()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("n", B_SIZES)
def test_unaligned_images_take_the_scalar_kernel_and_give_the_same_bits(n, name):
    """The same arrays in fresh allocations and as views one float into allocations of n + 1 -- all images, and each of
    them alone: the launch may use float4 accesses only where every image it touches is 16-byte aligned.  Both kinds of
    momentum step: the first, which writes the buffer, and a later one, which reads it."""
    tr = cases.trajectory(name, n, True, False)
    for first_step in (True, False) if tr["options"].get("momentum") else (True,):
        want = one_step(tr, False, first_step=first_step)
        assert not torch.equal(want["theta"], held(tr["theta0"]))
        present = Images(tr, False).present()
        assert ("vmax" in present) == bool(tr["options"].get("amsgrad")) and ("buf" in present) == bool(tr["options"].get("momentum"))
        for offsets in [tuple(present)] + [(image,) for image in present]:
            assert_same_bits(one_step(tr, False, offsets=offsets, first_step=first_step), want, f"offset {'+'.join(offsets)}")


@pytest.mark.parametrize("name", ADAM_SETS)
@pytest.mark.parametrize("linear", [False, True], ids=["log", "linear"])
@pytest.mark.parametrize("n", B_SIZES)
def test_device_bias_terms_give_the_bits_of_the_by_value_call(n, linear, name):
    """bias_dev = {step_size, bias2_sqrt} in device memory, NaN in the two fields of the options it replaces."""
    tr = cases.trajectory(name, n, True, linear)
    assert_same_bits(one_step(tr, linear, device_bias=True), one_step(tr, linear), "bias_dev")


MULTI_SIZES = [1, 2, 3, 64, 65, 200]


# no option set: what a session's small parameters take by default, held to the legacy single-tensor entries
PLAIN_SETS = {"plain-adam": (False, {}), "plain-sgd": (True, {})}
# (SGD has no bias terms)
MULTI_CASES = [pytest.param(name, device_bias, id=f"{name}-{'bias_dev' if device_bias else 'by-value'}")
               for name in SETS + sorted(PLAIN_SETS)
               for device_bias in ((False, True) if name in ADAM_SETS + ["plain-adam"] else (False,))]


@pytest.mark.parametrize("name,device_bias", MULTI_CASES)
def test_optimizer_step_multi_gives_the_single_tensor_bits(name, device_bias):
    """jd_optimizer_step_multi on tensors of ragged sizes, each at a step count of its own and -- momentum -- some on their
    first step (buffer NaN: written, not read) and some on a later one, against one jd_optimizer_step (linear, no mask) per
    tensor; with no option set against one jd_adam_step / jd_sgd_step per tensor."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, ptr_array, stream_ptr
    from jolideco_amd.ops import adam_bias_terms

    sgd, options = PLAIN_SETS[name] if name in PLAIN_SETS else cases.OPTION_SETS[name]
    lr = cases.learning_rate(sgd, True, options)
    rs = np.random.RandomState(37)
    counts = [1 + i % 5 for i in range(len(MULTI_SIZES))]
    firsts = [i % 2 == 0 for i in range(len(MULTI_SIZES))]
    tensors = []
    for n, first in zip(MULTI_SIZES, firsts):
        t = {"theta": rs.normal(size=n), "grad": rs.normal(size=n) * 10.0 ** rs.uniform(-3, 2, size=n)}
        if not sgd:
            t["m"], t["v"] = 0.1 * rs.normal(size=n), rs.uniform(size=n) ** 4
            if options.get("amsgrad"):
                t["vmax"] = t["v"] * rs.choice([0.5, 2.0], size=n)  # (either side of exp_avg_sq)
        elif options.get("momentum"):
            t["buf"] = np.full(n, NAN) if first else rs.normal(size=n)
        tensors.append({key: value.astype(np.float32) for key, value in t.items()})

    def device(t):
        return {key: held(value) for key, value in t.items()}

    singles = []
    for t, count, first in zip(tensors, counts, firsts):
        d = device(t)
        theta, size = ptr(d["theta"]), d["theta"].numel()
        if name == "plain-adam":
            step_size, bias2_sqrt = adam_bias_terms(count, lr, *cases.BETAS)
            beta1, beta2 = cases.BETAS
            check(_hip.lib().jd_adam_step(theta, theta, theta, ptr(d["grad"]), ptr(d["m"]), ptr(d["v"]), None, size, step_size, beta1,
                                          beta2, 1 - beta1, 1 - beta2, bias2_sqrt, cases.EPS, 0, 0, None, stream_ptr(DEV)))
        elif name == "plain-sgd":
            check(_hip.lib().jd_sgd_step(theta, theta, theta, ptr(d["grad"]), None, size, lr, 0, 0, stream_ptr(DEV)))
        else:
            args = options_struct(sgd, lr, options, count, first)
            check(_hip.lib().jd_optimizer_step(theta, theta, theta, ptr(d["grad"]), ptr(d.get("m")), ptr(d.get("v")), ptr(d.get("vmax")),
                                               ptr(d.get("buf")), None, size, ctypes.byref(args), 0, 0, None, stream_ptr(DEV)))
        singles.append(d)
    many = [device(t) for t in tensors]
    n = len(many)
    arrays = [ptr_array([d[key] for d in many]) if key in many[0] else None for key in ("theta", "grad", "m", "v", "vmax", "buf")]
    terms = [adam_bias_terms(c, lr, *cases.BETAS) for c in counts]
    by_value = [(NAN, NAN)] * n if device_bias else terms
    bias_dev = torch.tensor([x for t in terms for x in t], dtype=torch.float32, device=DEV) if device_bias else None
    args = options_struct(sgd, lr, options, by_value=False)
    check(_hip.lib().jd_optimizer_step_multi(
        n, *arrays, (ctypes.c_int * n)(*MULTI_SIZES), (ctypes.c_float * n)(*[t[0] for t in by_value]),
        (ctypes.c_float * n)(*[t[1] for t in by_value]), (ctypes.c_int * n)(*[int(f) for f in firsts]), ctypes.byref(args), ptr(bias_dev),
        stream_ptr(DEV)))
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(zip(many, singles)):
        for key in want:
            assert bool(torch.isfinite(want[key]).all()), (i, key)
            assert torch.equal(got[key], want[key]), f"tensor {i} (size {MULTI_SIZES[i]}): {key}"
        assert not torch.equal(got["theta"], held(tensors[i]["theta"]))


@pytest.mark.parametrize("optimizer_type", ["sgd", "adam"])
def test_step_parameters_gives_the_single_tensor_bits_and_skips_a_parameter_without_gradient(optimizer_type):
    """`core._step_parameters`, the step of a session's small parameters (one jd_optimizer_step_multi launch), on tensors of
    2, 1 and 5 floats of which the middle one has no gradient, twice: the stepped tensors carry the bits of one jd_sgd_step /
    jd_adam_step each, the parameter without gradient and its count are untouched, every other count advances by one."""
    from jolideco_amd import _hip, core
    from jolideco_amd._hip import check, ptr, stream_ptr
    from jolideco_amd.ops import adam_bias_terms

    cfg = core.MAPDeconvolver(device=DEV, optimizer_type=optimizer_type, display_progress=False)
    lr, (beta1, beta2) = cfg.optimizer_kwargs["lr"], cases.BETAS
    rs = np.random.RandomState(41)
    start = [rs.normal(size=n).astype(np.float32) for n in (2, 1, 5)]
    params = [torch.nn.Parameter(held(x)) for x in start]
    for p in (params[0], params[2]):
        p.grad = held(rs.normal(size=p.numel()).astype(np.float32))
    stepper = core._CalibrationStepper(params, cfg)
    want = [{"theta": held(x), "m": torch.zeros(x.size, device=DEV), "v": torch.zeros(x.size, device=DEV)} for x in start]
    cache = {}
    for count in (1, 2):
        core._step_parameters(cfg, list(zip(stepper.params, stepper.state)), cache)
        for i in (0, 2):
            w, n = want[i], start[i].size
            theta = ptr(w["theta"])
            if optimizer_type == "sgd":
                check(_hip.lib().jd_sgd_step(theta, theta, theta, ptr(params[i].grad), None, n, lr, 0, 0, stream_ptr(DEV)))
            else:
                step_size, bias2_sqrt = adam_bias_terms(count, lr, beta1, beta2)
                check(_hip.lib().jd_adam_step(theta, theta, theta, ptr(params[i].grad), ptr(w["m"]), ptr(w["v"]), None, n, step_size,
                                              beta1, beta2, 1 - beta1, 1 - beta2, bias2_sqrt, cases.EPS, 0, 0, None, stream_ptr(DEV)))
        torch.cuda.synchronize()
        assert [st["step"] for st in stepper.state] == [count, 0, count]
        for i, (p, st, w) in enumerate(zip(params, stepper.state, want)):
            assert bool(torch.isfinite(w["theta"]).all())
            assert torch.equal(p.data, w["theta"]), f"call {count}, tensor {i}: theta"
            assert torch.equal(st["exp_avg"], w["m"]) and torch.equal(st["exp_avg_sq"], w["v"]), f"call {count}, tensor {i}: moments"
        assert torch.equal(params[1].data, held(start[1])) and not torch.equal(params[0].data, held(start[0]))
    assert len(cache) == 1  # (the pointer arrays of the second call are those of the first)


PLAIN_MODES = {"adam-log": (False, False), "adam-linear": (False, True), "sgd-log": (True, False), "sgd-linear": (True, True)}


@pytest.mark.parametrize("keys", ["absent", "defaults"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("mode", sorted(PLAIN_MODES))
@pytest.mark.parametrize("n", B_SIZES)
def test_every_option_off_gives_the_bits_of_the_plain_step(n, mode, masked, keys):
    """jd_optimizer_step with no option set -- and with the state images of the options present all the same -- against
    jd_adam_step / jd_sgd_step on the trajectories of tests/optimizer_cases.py.  All three entries end in one launcher and
    one kernel (csrc/optimizer.hip): what this holds is that the legacy wrappers and jd_optimizer_step translate their
    arguments to the same launch.  The independent anchors of that kernel's bits are the fused steps of the gather and the
    band-sum kernel (tests/test_gpu_kernels.py) and the float64 / torch-bit checks of tests/test_gpu_optimizer_step.py."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, stream_ptr
    from jolideco_amd.ops import adam_bias_terms

    sgd, linear = PLAIN_MODES[mode]
    tr = plain_cases.trajectory(n, masked, linear, sgd)
    lr, (beta1, beta2), eps = tr["hyper"]
    assert (beta1, beta2, eps) == (*cases.BETAS, cases.EPS)
    step = tr["step0"] + 1
    as_option_case = {**tr, "sgd": sgd, "options": {}, "state0": {"exp_avg": tr["exp_avg0"], "exp_avg_sq": tr["exp_avg_sq0"]}}
    want, got = Images(as_option_case, linear), Images(as_option_case, linear)
    if sgd:
        check(_hip.lib().jd_sgd_step(ptr(want.theta), ptr(want.flux_in), ptr(want.flux_out), ptr(want.grad), ptr(want.mask), n, lr, 0,
                                     int(not linear), stream_ptr(DEV)))
    else:
        step_size, bias2_sqrt = adam_bias_terms(step, lr, beta1, beta2)
        check(_hip.lib().jd_adam_step(ptr(want.theta), ptr(want.flux_in), ptr(want.flux_out), ptr(want.grad), ptr(want.m), ptr(want.v),
                                      ptr(want.mask), n, step_size, beta1, beta2, 1 - beta1, 1 - beta2, bias2_sqrt, eps, 0, int(not linear),
                                      None, stream_ptr(DEV)))
    spare = torch.full((n,), 3.0, device=DEV)
    if keys == "defaults":
        got.vmax, got.buf = (spare, None) if not sgd else (None, spare)
    option_step(got, sgd=sgd, lr=lr, options={}, linear=linear, step=step, first_step=True)
    result = got.result()
    assert bool((spare == 3.0).all()), "a state image no option needs was touched"
    result.pop("max_exp_avg_sq", None), result.pop("momentum_buffer", None)
    assert_same_bits(result, want.result(), mode)
    assert not torch.equal(result["theta"], held(tr["theta0"]))


# ------------------------------------------------------------------------------------------------------------------
# C: sessions
# ------------------------------------------------------------------------------------------------------------------
def fit_inputs(golden, tag):
    from jolideco_amd import GMMPatchPrior, InverseGammaPrior, NPredCalibration, NPredCalibrations, SpatialFluxComponent
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    g = golden("optimizer_options")
    datasets = unpack_datasets(g, f"{tag}/data/")
    cals = NPredCalibrations()
    for name in datasets:
        sx, sy, norm, psf_scale = (float(v) for v in g[f"{tag}/cal_init/{name}"])
        cals[name] = NPredCalibration(shift_x=sx, shift_y=sy, background_norm=norm, psf_scale=psf_scale)
    if tag == "adam":
        gmm = GaussianMixtureModel.from_numpy(g["adam/gmm/means"], g["adam/gmm/covariances"], g["adam/gmm/weights"],
                                              meta=GaussianMixtureModelMeta(stride=4))
        prior = GMMPatchPrior(gmm=gmm)
    else:
        prior = InverseGammaPrior(alpha=10, beta=1.5)
    return g, datasets, SpatialFluxComponent.from_numpy(flux=g[f"{tag}/flux_init"], prior=prior), cals


def run_epochs(golden, tag, n_epochs, **config):
    """`n_epochs` epochs of a session on the inputs of fixture fit `tag`: (session, final theta, the epochs' scalars)."""
    from jolideco_amd import MAPDeconvolver

    _, datasets, comp, cals = fit_inputs(golden, tag)
    session = MAPDeconvolver(n_epochs=n_epochs, display_progress=False, device=DEV, **config).session(datasets, components=comp,
                                                                                                  calibrations=cals)
    rows = []
    for _ in range(n_epochs):
        session.epoch()
        rows.append(session.scalars.clone())
    torch.cuda.synchronize()
    parameters = [session.states[0].theta.clone()] + [p.data.clone() for opt in session.cal_optimizers for p in opt.params]
    return session, parameters, torch.stack(rows)


@pytest.mark.parametrize("optimizer_type,fit_mode", [("adam", "sequential"), ("sgd", "joint")])
def test_option_keys_at_their_defaults_change_no_bit_of_a_fit(golden, optimizer_type, fit_mode):
    from jolideco_amd.core import OPTIMIZER_OPTIONS

    config = dict(optimizer_type=optimizer_type, fit_mode=fit_mode, learning_rate=0.1 if optimizer_type == "adam" else 1e-3)
    plain, want, want_rows = run_epochs(golden, optimizer_type, 5, **config)
    keyed, got, rows = run_epochs(golden, optimizer_type, 5, optimizer_kwargs=dict(OPTIMIZER_OPTIONS[optimizer_type]), **config)
    assert torch.equal(rows, want_rows) and bool(torch.isfinite(rows).all())
    assert len(got) == len(want) == 5 and all(torch.equal(a, b) for a, b in zip(got, want))
    st, prior = keyed.states[0], keyed.priors[0]
    assert keyed._fuse_step(st, prior) == plain._fuse_step(st, prior)
    assert keyed.states[0].max_exp_avg_sq is None and keyed.states[0].momentum_buffer is None


def test_adam_option_fit_replayed_from_captured_epochs_equals_its_by_value_epochs(golden, monkeypatch):
    config = dict(optimizer_kwargs={"weight_decay": 1e-2, "amsgrad": True})
    monkeypatch.setenv("JOLIDECO_GRAPH", "0")
    eager, want, want_rows = run_epochs(golden, "adam", 10, **config)
    monkeypatch.setenv("JOLIDECO_GRAPH", "1")
    replayed, got, rows = run_epochs(golden, "adam", 10, **config)
    assert not eager._graphs and replayed._graphs and replayed._planned_capable()
    assert not replayed._fuse_step(replayed.states[0], replayed.priors[0])
    assert bool(replayed.states[0].max_exp_avg_sq.any()) and "max_exp_avg_sq" in replayed.cal_optimizers[0].state[0]
    assert torch.equal(rows, want_rows) and bool(torch.isfinite(rows).all())
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_a_momentum_fit_runs_by_value_epochs_only(golden, monkeypatch):
    monkeypatch.setenv("JOLIDECO_GRAPH", "1")
    session, parameters, rows = run_epochs(golden, "sgd", 6, optimizer_type="sgd", fit_mode="joint", learning_rate=1e-3,
                                           optimizer_kwargs={"momentum": 0.9, "nesterov": True})
    assert not session._planned_capable() and not session._graphs and session.step_scalars is None
    assert bool(session.states[0].momentum_buffer.any()) and not session.states[0].first_step
    assert all(not state["first_step"] and bool(state["momentum_buffer"].any()) for opt in session.cal_optimizers for state in opt.state)
    assert bool(torch.isfinite(rows).all())


# ------------------------------------------------------------------------------------------------------------------
# D: fits against the live reference
# ------------------------------------------------------------------------------------------------------------------
FITS = {
    "adam": dict(optimizer_kwargs={"weight_decay": 1e-2, "amsgrad": True}),
    "sgd": dict(fit_mode="joint", optimizer_type="sgd", learning_rate=1e-3, optimizer_kwargs={"momentum": 0.9, "nesterov": True}),
}


@pytest.mark.parametrize("tag", sorted(FITS))
def test_fit_with_options_matches_the_reference(golden, tag):
    """The plumbing of a fit with options -- which parameters step, their state, the order, the trace -- against the live
    reference: a sequential fit with the GMM prior under Adam {weight_decay, amsgrad}, a joint fit with the inverse-gamma
    prior under SGD {momentum, nesterov}; two observations with trainable calibrations, 6 epochs."""
    from jolideco_amd import MAPDeconvolver

    g, datasets, comp, cals = fit_inputs(golden, tag)
    res = MAPDeconvolver(n_epochs=int(g["n_epochs"]), display_progress=False, device=DEV, **FITS[tag]).run(
        datasets, components=comp, calibrations=cals)
    err = rel_linf(res.flux_upsampled_total, g[f"{tag}/flux_final"])
    print(f"\nfit {tag}: flux rel Linf {err:.2e}")
    for name in datasets:
        d = res.calibrations[name].to_dict()
        got = np.array([d["shift_x"], d["shift_y"], d["background_norm"], d["psf_scale"]])
        print(f"fit {tag}: calibration {name} |gpu - ref| {np.abs(got - g[f'{tag}/cal_final/{name}']).max():.2e}")
    assert err < 1e-5
    for key, ref in g.items():
        if key.startswith(f"{tag}/trace/"):
            name = key[len(f"{tag}/trace/"):]
            np.testing.assert_allclose(res.trace_loss[name], ref, rtol=2e-5, atol=1e-6, err_msg=name)
    for name in datasets:
        d = res.calibrations[name].to_dict()
        got = np.array([d["shift_x"], d["shift_y"], d["background_norm"], d["psf_scale"]])
        np.testing.assert_allclose(got, g[f"{tag}/cal_final/{name}"], rtol=2e-4, atol=2e-5, err_msg=name)
        assert not np.array_equal(got[:3], g[f"{tag}/cal_init/{name}"][:3])

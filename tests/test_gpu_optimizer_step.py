"""GPU: every kernel that ends in csrc/jd_adam.h's `adam_pixel` / `adam_update`.

A  the plain step (jd_adam_step, jd_sgd_step; log and linear flux, with and without mask, the float4 and the scalar kernel,
   the second trip of their grid-stride loops) against torch.optim in float64 (tests/optimizer_cases.py), mid-trajectory,
   under bound() of the float32 oracle's own error: theta and the moments by relative L-inf, the flux per pixel.
B  variants that must give the plain step's bits: unaligned images (scalar kernel), the device-resident bias terms,
   jd_adam_step_multi, addend images, theta / flux_in / flux_out in one buffer.
C  the fused steps (jd_gmm_prior_fwd_bwd_step in the tiled gather kernel -- the per-pixel one has no step and the entry
   refuses it; jd_add_rolled_bands_step) against prior-then-step bit for bit, in the variants no fit reaches, and once
   each against float64.

Largest figures of part A and of the float64 ties of part C on an MI355X (kernel | float32 oracle, both against float64):
  adam-log    : theta 1.44e-07 | 1.44e-07, exp_avg 2.22e-07 | 2.22e-07, exp_avg_sq 2.42e-07 | 2.42e-07, flux 7.59e-07 | 7.59e-07
  adam-linear : theta 1.28e-07 | 1.28e-07, exp_avg 1.31e-07 | 5.98e-08, exp_avg_sq 1.35e-07 | 1.29e-07, flux 9.66e-02 | 3.45e-02
  sgd-log     : theta 1.24e-07 | 1.24e-07, flux 5.94e-07 | 5.94e-07
  sgd-linear  : theta 1.02e-07 | 1.02e-07, flux 6.40e-03 | 6.40e-03
  fused gmm   : theta 3.46e-08 | 3.43e-08, exp_avg 8.29e-08 | 4.08e-08, exp_avg_sq 9.75e-08 | 9.75e-08, flux 1.66e-07 | 1.59e-07
  fused bands : theta 3.53e-08 | 3.53e-08, exp_avg 4.55e-08 | 4.55e-08, exp_avg_sq 4.01e-08 | 4.01e-08, flux 1.50e-07 | 1.50e-07
(The per-pixel flux error of a LINEAR parameter is large in both columns where a step lands next to zero, at the million
pixel sizes: a rounding of the update against a flux a million times smaller.  The SGD update was a product and a
difference rounded apart and came out at 4.1 to 4.3 x the oracle there -- 9.83e-06 | 2.28e-06 at n = 3072, 1.21e-03 |
2.97e-04 at n = 1 048 835 -- until jd_adam.h took torch's fused multiply-add.)
With addend images the library's own two calls (prior into the gradient image, then jd_adam_step_addends) add the prior's
term BEFORE the addends, the fused kernel after them: theta differs in 12 to 53 of the 1961 / 2560 pixels of the shapes below.
"""
import ctypes

import numpy as np
import pytest
import torch

import optimizer_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MODES = {"adam-log": (False, False), "adam-linear": (False, True), "sgd-log": (True, False), "sgd-linear": (True, True)}
IMAGES = ("theta", "flux_in", "flux_out", "grad", "m", "v", "mask")  # the seven pointers of a step
KEYS = ("theta", "flux", "exp_avg", "exp_avg_sq")


def held(array, offset=False, shape=None):
    """`array` in a fresh device allocation, or (`offset`) as a view one float into an allocation of n + 1: 4-byte aligned."""
    if array is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)).reshape(-1)
    buf = torch.empty(src.numel() + int(offset), device=DEV)
    view = buf[int(offset):]
    view.copy_(src)
    assert view.data_ptr() % 16 == (4 if offset else 0) and view.is_contiguous()
    return view if shape is None else view.reshape(shape)


class State:
    """The images of one optimizer step on the device, as step `step0` of a trajectory left them: flux_in =
    exp(theta) * mask (linear: theta * mask)."""

    def __init__(self, tr, linear, shape=None, offsets=(), grad=None):
        flux = tr["theta0"].astype(np.float32) if linear else np.exp(tr["theta0"].astype(np.float64)).astype(np.float32)
        if tr["mask"] is not None:
            flux = flux * tr["mask"]
        mk = lambda name, a: held(a, name in offsets, shape)  # noqa: E731
        self.theta, self.flux_in, self.flux_out = mk("theta", tr["theta0"]), mk("flux_in", flux), mk("flux_out", np.full_like(flux, NAN))
        self.grad = mk("grad", tr["grads"][0] if grad is None else grad)
        self.m, self.v, self.mask = mk("m", tr["exp_avg0"]), mk("v", tr["exp_avg_sq0"]), mk("mask", tr["mask"])
        self.n = self.theta.numel()

    def result(self):
        torch.cuda.synchronize()
        return {"theta": self.theta.clone(), "flux": self.flux_out.clone(), "exp_avg": None if self.m is None else self.m.clone(),
                "exp_avg_sq": None if self.v is None else self.v.clone()}


def bias_terms(step, hyper, device_bias):
    """(step_size, bias2_sqrt, bias_dev): by value, or in device memory with NaN in the by-value arguments."""
    from jolideco_amd.ops import adam_bias_terms

    lr, (beta1, beta2), _ = hyper
    step_size, bias2_sqrt = adam_bias_terms(step, lr, beta1, beta2)
    if not device_bias:
        return step_size, bias2_sqrt, None
    return NAN, NAN, torch.tensor([step_size, bias2_sqrt], dtype=torch.float32, device=DEV)


def plain_step(s, *, sgd, linear, hyper, step, zero_grad=0, device_bias=False, addends=None):
    """jd_sgd_step / jd_adam_step / jd_adam_step_addends on the images of `s`."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, ptr_array, stream_ptr

    lr, (beta1, beta2), eps = hyper
    if sgd:
        check(_hip.lib().jd_sgd_step(ptr(s.theta), ptr(s.flux_in), ptr(s.flux_out), ptr(s.grad), ptr(s.mask), s.n, lr, zero_grad,
                                     int(not linear), stream_ptr(DEV)))
    else:
        step_size, bias2_sqrt, bias_dev = bias_terms(step, hyper, device_bias)
        args = (ptr(s.theta), ptr(s.flux_in), ptr(s.flux_out), ptr(s.grad), ptr(s.m), ptr(s.v), ptr(s.mask), s.n, step_size, beta1,
                beta2, 1 - beta1, 1 - beta2, bias2_sqrt, eps, zero_grad, int(not linear), ptr(bias_dev))
        if addends is None:
            check(_hip.lib().jd_adam_step(*args, stream_ptr(DEV)))
        else:
            padded = list(addends) + [None] * (_hip.ADDEND_MAX - len(addends))
            check(_hip.lib().jd_adam_step_addends(*args, ptr_array(padded), stream_ptr(DEV)))
    torch.cuda.synchronize()


def fill_step(s, *, sgd, linear, hyper, step, device_bias=False, addends=()):
    """The `jd_step` of the fused entries for the images of `s` (returns it with what must stay alive)."""
    from jolideco_amd import _hip

    lr, (beta1, beta2), eps = hyper
    step_size, bias2_sqrt, bias_dev = (0.0, 1.0, None) if sgd else bias_terms(step, hyper, device_bias)
    address = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = _hip.Step(theta=address(s.theta), flux_in=address(s.flux_in), flux_out=address(s.flux_out), grad_flux=address(s.grad),
                   exp_avg=address(s.m), exp_avg_sq=address(s.v), mask=address(s.mask), step_size=step_size, beta1=beta1,
                   beta2=beta2, one_minus_beta1=1 - beta1, one_minus_beta2=1 - beta2, bias2_sqrt=bias2_sqrt, eps=eps, lr=lr,
                   use_log_flux=int(not linear), sgd=int(sgd), bias_dev=address(bias_dev))
    for k, image in enumerate(addends):
        st.addend[k] = address(image)
    return st, (bias_dev, addends)


def assert_same_bits(got, want, label):
    for key in KEYS:
        if want[key] is None:
            assert got[key] is None
            continue
        assert bool(torch.isfinite(want[key]).all()), f"{label}: {key} of the plain step is not finite"
        assert torch.equal(got[key], want[key]), (
            f"{label}: {key} differs in {int((got[key] != want[key]).sum())} of {want[key].numel()} pixels")


def assert_within_oracle_bounds(got, tr, label, steps=None, ref64=None, ref32=None):
    """`got` (as cases.oracle returns it) against the float64 oracle under bound() of the float32 oracle's own error, step
    by step and quantity by quantity; prints the largest figure of each quantity beside the oracle's own."""
    ref64, ref32 = ref64 or tr["ref64"], ref32 or tr["ref32"]
    worst, failures = {}, []
    for step in range(len(got["theta"]) if steps is None else steps):
        err, own = cases.errors(got, ref64, tr["mask"], step), cases.errors(ref32, ref64, tr["mask"], step)
        for key in err:
            if key not in worst or err[key] > worst[key][0]:
                worst[key] = (err[key], own[key])
            if not err[key] <= cases.bound(own[key]):
                failures.append(f"step {step} {key}: {err[key]:.3e} > bound({own[key]:.3e}) = {cases.bound(own[key]):.3e}")
    print(f"\n{label}: " + ", ".join(f"{key} {e:.2e} | {o:.2e}" for key, (e, o) in worst.items()))
    assert not failures, f"{label}: " + "; ".join(failures)


# ------------------------------------------------------------------------------------------------------------------
# A: the plain step against float64
# ------------------------------------------------------------------------------------------------------------------
SMALL_SIZES = (4, 1020, 1021)  # one thread | float4 kernel, ragged last wave | scalar kernel
# whole blocks | second trip of the scalar kernel's grid-stride loop (4096 blocks x 256 pixels)
OTHER_SIZES = (256 * 4 * 3, (1 << 20) + 259)
VECTOR_SECOND_TRIP = (1 << 22) + 1024  # second trip of the float4 kernel's loop (4096 blocks x 1024 pixels)


def plain_cases():
    out = []

    def add(mode, masked, n, hyper, n_steps, zero_grad):
        out.append(pytest.param(mode, masked, n, hyper, n_steps, zero_grad,
                                id=f"{mode}-{'mask' if masked else 'nomask'}-n{n}-{hyper}-zero_grad{zero_grad}"))

    for n in SMALL_SIZES + OTHER_SIZES:
        for hyper in ("default", "other") if n in SMALL_SIZES else ("default",):
            for mode in MODES:
                for masked in (False, True):
                    for zero_grad in (0, 1):  # (innermost: both cases share one cached trajectory)
                        add(mode, masked, n, hyper, 4, zero_grad)
    for masked in (False, True):
        for zero_grad in (0, 1):
            add("adam-log", masked, VECTOR_SECOND_TRIP, "default", 2, zero_grad)
    return out


@pytest.mark.parametrize("mode,masked,n,hyper,n_steps,zero_grad", plain_cases())
def test_plain_step_matches_torch_optim_in_float64(mode, masked, n, hyper, n_steps, zero_grad):
    """jd_adam_step / jd_sgd_step from the moments and the step count of a three-step warm-up, `n_steps` steps with fresh
    gradients, each on the flux the step before left: theta, both moments and the flux after every step against the float64
    oracle; masked pixels keep theta bit for bit and have flux exactly 0; the gradient image is zeroed or left alone."""
    sgd, linear = MODES[mode]
    tr = cases.trajectory(n, masked, linear, sgd, hyper, n_steps)
    s = State(tr, linear)
    start = s.theta.clone()
    got = {key: [] for key in tr["ref64"]}
    for i in range(n_steps):
        s.grad = held(tr["grads"][i])
        before = s.grad.clone()
        plain_step(s, sgd=sgd, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1 + i, zero_grad=zero_grad)
        if zero_grad:
            assert not bool(s.grad.any()), "zero_grad = 1 left a gradient"
        else:
            assert torch.equal(s.grad.view(torch.int32), before.view(torch.int32)), "zero_grad = 0 changed the gradient image"
        res = s.result()
        for key in got:
            got[key].append(res[key].cpu().numpy())
        if masked:
            off = s.mask == 0
            assert bool((res["flux"][off] == 0).all()), f"step {i}: flux under the mask"
            assert torch.equal(res["theta"][off].view(torch.int32), start[off].view(torch.int32)), f"step {i}: a masked theta moved"
        s.flux_in, s.flux_out = s.flux_out, s.flux_in
    assert n <= 4 or not torch.equal(s.theta, start)
    assert_within_oracle_bounds(got, tr, f"{mode} {'mask' if masked else 'nomask'} n={n} {hyper} zero_grad={zero_grad}")


# ------------------------------------------------------------------------------------------------------------------
# B: variants that must give the plain step's bits
# ------------------------------------------------------------------------------------------------------------------
B_SIZES = (1020, 1021)
mask_ids = pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
size_ids = pytest.mark.parametrize("n", B_SIZES)


def one_plain_step(tr, sgd, linear, **kw):
    s = State(tr, linear, offsets=kw.pop("offsets", ()))
    plain_step(s, sgd=sgd, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1, **kw)
    return s.result()


@pytest.mark.parametrize("mode", sorted(MODES))
@mask_ids
@size_ids
def test_unaligned_images_take_the_scalar_kernel_and_give_the_same_bits(n, masked, mode):
    """The same arrays in fresh allocations and as views one float into allocations of n + 1 -- all seven images, and each
    of them alone: the launch may use float4 accesses only where every image is 16-byte aligned."""
    sgd, linear = MODES[mode]
    tr = cases.trajectory(n, masked, linear, sgd)
    want = one_plain_step(tr, sgd, linear)
    assert not torch.equal(want["theta"], held(tr["theta0"]))
    present = [name for name in IMAGES if not (sgd and name in ("m", "v")) and not (name == "mask" and not masked)]
    for offsets in [tuple(present)] + [(name,) for name in present]:
        assert_same_bits(one_plain_step(tr, sgd, linear, offsets=offsets), want, f"offset {'+'.join(offsets)}")


@pytest.mark.parametrize("linear", [False, True], ids=["log", "linear"])
@mask_ids
@size_ids
def test_device_bias_terms_give_the_bits_of_the_by_value_call(n, masked, linear):
    """bias_dev = {step_size, bias2_sqrt} in device memory, NaN in the two by-value arguments it replaces."""
    tr = cases.trajectory(n, masked, linear, False)
    want = one_plain_step(tr, False, linear)
    assert_same_bits(one_plain_step(tr, False, linear, device_bias=True), want, "bias_dev")


def multi_step(thetas, grads, ms, vs, terms, hyper, device_bias):
    from jolideco_amd import _hip
    from jolideco_amd._hip import ptr, ptr_array, stream_ptr

    _, (beta1, beta2), eps = hyper
    n = len(thetas)
    sizes = (ctypes.c_int * n)(*[t.numel() for t in thetas])
    by_value = [NAN] * n if device_bias else None
    step_size = (ctypes.c_float * n)(*(by_value or [t[0] for t in terms]))
    bias2_sqrt = (ctypes.c_float * n)(*(by_value or [t[1] for t in terms]))
    bias_dev = torch.tensor([x for t in terms for x in t], dtype=torch.float32, device=DEV) if device_bias else None
    status = _hip.lib().jd_adam_step_multi(n, ptr_array(thetas), ptr_array(grads), ptr_array(ms), ptr_array(vs), sizes, step_size,
                                           bias2_sqrt, beta1, beta2, 1 - beta1, 1 - beta2, eps, ptr(bias_dev), stream_ptr(DEV))
    torch.cuda.synchronize()
    return status


@pytest.mark.parametrize("sizes", [[1, 2, 3, 64, 65, 200], [2] * 64], ids=["ragged", "64x2"])
@pytest.mark.parametrize("hyper", sorted(cases.HYPER))
def test_adam_step_multi_by_value_and_device_bias_give_the_single_tensor_bits(sizes, hyper):
    """jd_adam_step_multi with the bias terms by value and with bias_dev of 2 n floats (NaN by value), every tensor at a
    step count of its own, against one jd_adam_step (linear, no mask) per tensor; 64 tensors are the most it takes."""
    from jolideco_amd._hip import check
    from jolideco_amd.ops import adam_bias_terms

    hp = cases.HYPER[hyper]
    lr, (beta1, beta2), _ = hp
    rs = np.random.RandomState(31)
    arrays = [{"theta0": rs.normal(size=n).astype(np.float32), "exp_avg0": (0.1 * rs.normal(size=n)).astype(np.float32),
               "exp_avg_sq0": (rs.uniform(size=n) ** 4).astype(np.float32), "mask": None,
               "grads": [(rs.normal(size=n) * 10.0 ** rs.uniform(-3, 2, size=n)).astype(np.float32)]} for n in sizes]
    counts = [1 + i % 7 for i in range(len(sizes))]
    terms = [adam_bias_terms(c, lr, beta1, beta2) for c in counts]
    single = []
    for tr, count in zip(arrays, counts):
        s = State(tr, True)
        plain_step(s, sgd=False, linear=True, hyper=hp, step=count)
        single.append(s.result())
    for device_bias in (False, True):
        states = [State(tr, True) for tr in arrays]
        check(multi_step([s.theta for s in states], [s.grad for s in states], [s.m for s in states], [s.v for s in states], terms, hp,
                         device_bias))
        for i, (s, want) in enumerate(zip(states, single)):
            for key, image in (("theta", s.theta), ("exp_avg", s.m), ("exp_avg_sq", s.v)):
                assert torch.equal(image, want[key]), f"tensor {i} (size {sizes[i]}), device_bias={device_bias}: {key}"
            assert not torch.equal(s.theta, held(arrays[i]["theta0"]))


def test_adam_step_multi_refuses_more_than_64_tensors():
    from jolideco_amd import _hip

    tensors = [torch.zeros(2, device=DEV) for _ in range(65)]
    terms = [(0.1, 1.0)] * 65
    assert multi_step(tensors, tensors, tensors, tensors, terms, cases.HYPER["default"], False) == -1
    assert b"not in [1, 64]" in _hip.lib().jd_last_error()
    assert not any(bool(t.any()) for t in tensors)


@pytest.mark.parametrize("linear", [False, True], ids=["log", "linear"])
@mask_ids
@size_ids
def test_addend_images_give_the_bits_of_the_step_on_their_sum(n, masked, linear):
    """jd_adam_step_addends with 1 to 4 images against jd_adam_step on ((grad + a0) + a1) + ... summed by torch in float32
    in that order; a null entry ends the list; an image that is only 4-byte aligned changes no bit."""
    tr = cases.trajectory(n, masked, linear, False)
    rs = np.random.RandomState(n + 7)
    images = [(rs.normal(size=n) * 10.0 ** rs.uniform(-3, 2, size=n)).astype(np.float32) for _ in range(4)]
    wants = []
    for k in range(1, 5):
        total = held(tr["grads"][0])
        for image in images[:k]:
            total = total + held(image)
        s = State(tr, linear)
        s.grad = total
        plain_step(s, sgd=False, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1)
        wants.append(s.result())
        got = one_plain_step(tr, False, linear, addends=[held(image) for image in images[:k]])
        assert_same_bits(got, wants[-1], f"{k} addends")
        if k > 1:
            assert not torch.equal(wants[-1]["theta"], wants[-2]["theta"])
        unaligned = [held(image, offset=(j == k - 1)) for j, image in enumerate(images[:k])]
        assert_same_bits(one_plain_step(tr, False, linear, addends=unaligned), wants[-1], f"{k} addends, the last 4-byte aligned")
    ended = one_plain_step(tr, False, linear, addends=[held(images[0]), None, held(images[2])])
    assert_same_bits(ended, wants[0], "a null entry between two images")
    s = State(tr, linear)
    plain_step(s, sgd=False, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1, addends=[held(images[0])])
    assert torch.equal(s.grad, held(tr["grads"][0])), "the step wrote to its gradient image"


@pytest.mark.parametrize("sgd", [False, True], ids=["adam", "sgd"])
@mask_ids
@size_ids
def test_linear_step_in_one_buffer_gives_the_bits_of_the_three_buffer_call(n, masked, sgd):
    """theta, flux_in and flux_out in ONE buffer (linear parameters: how the calibration parameters are stepped).  The
    flux is written last, so the buffer ends as the three-buffer call's flux; without a mask that is its theta too."""
    tr = cases.trajectory(n, masked, True, sgd)
    want = one_plain_step(tr, sgd, True)
    s = State(tr, True)
    s.flux_in = s.flux_out = s.theta
    plain_step(s, sgd=sgd, linear=True, hyper=tr["hyper"], step=tr["step0"] + 1)
    got = s.result()
    assert torch.equal(got["theta"], want["flux"])
    on = slice(None) if not masked else s.mask != 0
    assert torch.equal(got["theta"][on], want["theta"][on])
    if not sgd:
        assert torch.equal(got["exp_avg"], want["exp_avg"]) and torch.equal(got["exp_avg_sq"], want["exp_avg_sq"])


# ------------------------------------------------------------------------------------------------------------------
# C: the fused steps against prior-then-step
# ------------------------------------------------------------------------------------------------------------------
OPTIMIZERS = {"adam": (False, False), "adam-bias_dev": (False, True), "sgd": (True, False)}  # (sgd, device_bias)
FLUX_MASK = [(linear, masked) for linear in (False, True) for masked in (False, True)]
# (shape, shifts): aligned groups of four | groups that straddle the border and go pixel by pixel | W % 4 != 0, and a last row
# and column of the rolled frame under no patch
GMM_GEOMETRIES = {"40x64": ((40, 64), (0, 0)), "40x64-rolled": ((40, 64), (1, -3)), "37x53-rolled": ((37, 53), (2, 1))}
STRIDE = 4


@pytest.fixture(scope="module")
def gmm_handle():
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
    from oracle import cpu_ref

    means, covs, weights = cpu_ref.synthetic_gmm(4, 64, seed=2)
    gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=STRIDE))
    return gmm.handle(DEV)


def gmm_unfused(handle, tr, shape, shifts, *, sgd, linear, addends=(), library_order=False):
    """The prior's gradient accumulated into the gradient image, then the plain step.  With addends: into
    (grad + a0) + a1 ..., the order of the fused kernel; `library_order`: into grad, the addends left to
    jd_adam_step_addends.  Returns (result, prior value, the gradient the step consumed)."""
    s = State(tr, linear, shape)
    value = torch.full((1,), NAN, device=DEV)
    if not library_order:
        for image in addends:
            s.grad = s.grad + image
    scale = 1.0 / s.n
    handle.prior_fwd_bwd(s.flux_in, STRIDE, shifts, value, scale, grad=s.grad, grad_coef=-0.7 * scale)
    consumed = s.grad.clone()
    plain_step(s, sgd=sgd, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1,
               addends=list(addends) if library_order and addends else None)
    return s.result(), value, consumed


def gmm_fused(handle, tr, shape, shifts, *, sgd, linear, device_bias=False, addends=(), offsets=()):
    s = State(tr, linear, shape, offsets=offsets)
    before = s.grad.clone()
    value = torch.full((1,), NAN, device=DEV)
    st, alive = fill_step(s, sgd=sgd, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1, device_bias=device_bias, addends=addends)
    scale = 1.0 / s.n
    handle.prior_fwd_bwd_step(s.flux_in, STRIDE, shifts, value, scale, -0.7 * scale, st)
    result = s.result()
    assert torch.equal(s.grad, before), "the fused step wrote to its gradient image"
    del alive
    return result, value


# (jd_adam_step_addends, the unfused side of a step with addend images, has no SGD form)
GMM_CASES = [pytest.param(geometry, optimizer, n_addends, id=f"{geometry}-{optimizer}-{n_addends}addends")
             for geometry in sorted(GMM_GEOMETRIES) for optimizer in sorted(OPTIMIZERS) for n_addends in (0, 1, 2)
             if not (OPTIMIZERS[optimizer][0] and n_addends)]


@pytest.mark.parametrize("geometry,optimizer,n_addends", GMM_CASES)
def test_step_in_the_gather_kernel_gives_the_bits_of_prior_then_step(gmm_handle, geometry, optimizer, n_addends):
    """jd_gmm_prior_fwd_bwd_step against jd_gmm_prior_fwd_bwd into the gradient image followed by the plain step: theta,
    flux, both moments and the prior's value, for log and linear flux, with and without mask.  With addend images the
    unfused side adds them to the gradient first, the fused kernel's order; how many pixels the library's own two calls
    (prior into the gradient image, then jd_adam_step_addends: the prior's term BEFORE the addends) change is printed."""
    shape, shifts = GMM_GEOMETRIES[geometry]
    sgd, device_bias = OPTIMIZERS[optimizer]
    n = shape[0] * shape[1]
    rs = np.random.RandomState(n + n_addends)
    addends = [held((rs.normal(size=n) * 10.0 ** rs.uniform(-3, 2, size=n)).astype(np.float32), shape=shape) for _ in range(n_addends)]
    for linear, masked in FLUX_MASK:
        label = f"{'linear' if linear else 'log'} {'mask' if masked else 'nomask'}"
        tr = cases.trajectory(n, masked, linear, sgd)
        want, want_value, consumed = gmm_unfused(gmm_handle, tr, shape, shifts, sgd=sgd, linear=linear, addends=addends)
        got, value = gmm_fused(gmm_handle, tr, shape, shifts, sgd=sgd, linear=linear, device_bias=device_bias, addends=addends)
        assert_same_bits(got, want, label)
        assert bool(torch.isfinite(want_value).all()) and torch.equal(value, want_value), f"{label}: prior value"
        plain = State(tr, linear, shape)
        assert not torch.equal(consumed, plain.grad), "the prior added nothing to the gradient"
        assert not torch.equal(want["theta"], plain.theta)
        if addends:
            library, _, _ = gmm_unfused(gmm_handle, tr, shape, shifts, sgd=sgd, linear=linear, addends=addends, library_order=True)
            differ = int((library["theta"] != got["theta"]).sum())
            print(f"\n{geometry} {optimizer} {label}, {n_addends} addends: prior-then-jd_adam_step_addends differs from the fused "
                  f"step in theta at {differ} of {n} pixels")


def test_fused_gather_step_is_refused_where_the_per_pixel_gather_kernel_is_selected(gmm_handle, jd_option):
    """JD_GMM_GATHER_TILED = 0 selects the per-pixel gather kernel, which has no optimizer step: the fused entry returns
    JD_ERR_INVALID before it launches anything (the session then makes the two calls) and leaves every image alone."""
    jd_option("JD_GMM_GATHER_TILED", 0)
    shape, shifts = GMM_GEOMETRIES["40x64"]
    tr = cases.trajectory(shape[0] * shape[1], True, False, False)
    s, untouched = State(tr, False, shape), State(tr, False, shape)
    st, alive = fill_step(s, sgd=False, linear=False, hyper=tr["hyper"], step=tr["step0"] + 1)
    value = torch.full((1,), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="jd_gmm_prior_fwd_bwd_step"):
        gmm_handle.prior_fwd_bwd_step(s.flux_in, STRIDE, shifts, value, 1.0 / s.n, -0.7 / s.n, st)
    torch.cuda.synchronize()
    for name in ("theta", "flux_out", "grad", "m", "v"):
        assert torch.equal(getattr(s, name).view(torch.int32), getattr(untouched, name).view(torch.int32)), name
    assert float(value) == 3.0
    del alive


def test_gather_kernel_steps_the_pixels_no_patch_covers(gmm_handle):
    """(37, 53) rolled by (2, 1): the last row and the last column of the rolled frame lie under no patch; their pixels take
    the likelihood gradient alone and are stepped all the same."""
    shape, shifts = GMM_GEOMETRIES["37x53-rolled"]
    tr = cases.trajectory(shape[0] * shape[1], False, False, False)
    plain = State(tr, False, shape)
    plain_step(plain, sgd=False, linear=False, hyper=tr["hyper"], step=tr["step0"] + 1)
    want = plain.result()
    got, _ = gmm_fused(gmm_handle, tr, shape, shifts, sgd=False, linear=False)
    bare = torch.zeros(shape, dtype=torch.bool, device=DEV)
    bare[(36 - shifts[0]) % shape[0], :] = True  # rolled row 36 / column 52 in the un-rolled image
    bare[:, (52 - shifts[1]) % shape[1]] = True
    for key in KEYS:
        assert torch.equal(got[key][bare], want[key][bare]), key
    assert not torch.equal(got["theta"][~bare], want["theta"][~bare])


@pytest.mark.parametrize("name", ["grad", "theta", "flux_out", "m", "mask"])
def test_fused_gather_step_with_one_unaligned_image_gives_the_same_bits(gmm_handle, name):
    """One of the step's images only 4-byte aligned: the gather kernel steps pixel by pixel."""
    shape, shifts = GMM_GEOMETRIES["40x64"]
    tr = cases.trajectory(shape[0] * shape[1], True, False, False)
    want, want_value = gmm_fused(gmm_handle, tr, shape, shifts, sgd=False, linear=False)
    got, value = gmm_fused(gmm_handle, tr, shape, shifts, sgd=False, linear=False, offsets=(name,))
    assert_same_bits(got, want, f"offset {name}")
    assert torch.equal(value, want_value)


def one_step_oracles(tr, grad):
    """The float64 and the float32 oracle for ONE log-flux Adam step from the start of `tr` on the gradient `grad`."""
    lr, betas, eps = tr["hyper"]
    kw = dict(linear=False, sgd=False, lr=lr, betas=betas, eps=eps, exp_avg0=tr["exp_avg0"], exp_avg_sq0=tr["exp_avg_sq0"],
              step0=tr["step0"])
    return {name: cases.oracle(tr["theta0"], tr["mask"], [np.asarray(grad).ravel()], dtype=dtype, **kw)
            for name, dtype in (("ref64", torch.float64), ("ref32", torch.float32))}


BAND_SHAPE = (24, 64)
BAND_ROWS = [(2, 13), (11, 22), (5, 5)]  # two bands that share rows 11 and 12, an empty one; rows 0, 1, 22, 23 under none
BAND_CHUNK = 11 * 64


def band_buffer():
    rs = np.random.RandomState(77)
    return held((rs.normal(size=3 * BAND_CHUNK) * 10.0 ** rs.uniform(-3, 2, size=3 * BAND_CHUNK)).astype(np.float32))


def bands_unfused(tr, shifts, *, sgd, linear):
    from jolideco_amd import ops

    s = State(tr, linear, BAND_SHAPE)
    ops.add_rolled_bands(s.grad, shifts, band_buffer(), BAND_CHUNK, BAND_ROWS)
    consumed = s.grad.clone()
    plain_step(s, sgd=sgd, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1)
    return s.result(), consumed


def bands_fused(tr, shifts, *, sgd, linear, device_bias=False):
    from jolideco_amd import ops

    s = State(tr, linear, BAND_SHAPE)
    before = s.grad.clone()
    st, alive = fill_step(s, sgd=sgd, linear=linear, hyper=tr["hyper"], step=tr["step0"] + 1, device_bias=device_bias)
    ops.add_rolled_bands_step(BAND_SHAPE, shifts, band_buffer(), BAND_CHUNK, BAND_ROWS, st)
    result = s.result()
    assert torch.equal(s.grad, before), "the fused step wrote to its gradient image"
    del alive
    return result


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
@pytest.mark.parametrize("shifts", [(5, -7), (0, 0)], ids=["rolled", "unrolled"])
def test_step_inside_the_band_sum_gives_the_bits_of_sum_then_step(shifts, optimizer):
    """jd_add_rolled_bands_step against jd_add_rolled_bands followed by the plain step, for log and linear flux, with and
    without mask: overlapping bands, an empty band, rows no band holds."""
    sgd, device_bias = OPTIMIZERS[optimizer]
    n = BAND_SHAPE[0] * BAND_SHAPE[1]
    for linear, masked in FLUX_MASK:
        tr = cases.trajectory(n, masked, linear, sgd)
        want, consumed = bands_unfused(tr, shifts, sgd=sgd, linear=linear)
        got = bands_fused(tr, shifts, sgd=sgd, linear=linear, device_bias=device_bias)
        assert_same_bits(got, want, f"{'linear' if linear else 'log'} {'mask' if masked else 'nomask'}")
        plain = State(tr, linear, BAND_SHAPE)
        changed = (consumed != plain.grad).any(dim=1)
        assert int(changed.sum()) == 20 and not torch.equal(want["theta"], plain.theta)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("entry", ["gmm", "bands"])
def test_fused_log_flux_adam_steps_match_float64(gmm_handle, entry, masked):
    """The fused entries' log-flux Adam step against the float64 oracle on the gradient the unfused run consumed, under the
    bounds of the plain step: equality with the plain step alone would pass an error the callers of adam_pixel share."""
    if entry == "bands":
        shape, shifts = BAND_SHAPE, (5, -7)
        tr = cases.trajectory(shape[0] * shape[1], masked, False, False)
        _, consumed = bands_unfused(tr, shifts, sgd=False, linear=False)
        fused = bands_fused(tr, shifts, sgd=False, linear=False)
    else:
        shape, shifts = GMM_GEOMETRIES["40x64-rolled"]
        tr = cases.trajectory(shape[0] * shape[1], masked, False, False)
        _, _, consumed = gmm_unfused(gmm_handle, tr, shape, shifts, sgd=False, linear=False)
        fused, _ = gmm_fused(gmm_handle, tr, shape, shifts, sgd=False, linear=False)
    refs = one_step_oracles(tr, consumed.cpu().numpy())
    got = {key: [fused[key].cpu().numpy().ravel()] for key in KEYS}
    assert_within_oracle_bounds(got, tr, f"fused {entry} {'mask' if masked else 'nomask'}", **refs)
    if masked:
        off = tr["mask"] == 0
        assert np.all(got["flux"][0][off] == 0) and np.array_equal(got["theta"][0][off], tr["theta0"][off])

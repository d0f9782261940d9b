"""GPU: every instantiation of the MFMA Toeplitz kernel (csrc/directconv.hip: direct_conv_kernel<KC, VEC, POISSON, SPLIT>)
against float64.  Every case first asks `ConvPlan.direct_kernel` (jd_conv_plan_direct_kernel) which instantiation its plan
launches and asserts that it is the one the case is meant for.

A  the first and the last PSF width of every KC class, kh in {1, 2, 9, 33}, the fp32 kernel (JD_DIRECT_FP32=1) and the
   split-fp16 one, a width that stages float4 (70 x 76) and one that stages scalars (70 x 75); forward with / without the
   scale image, adjoint written into NaNs and accumulated, with / without the scale image.
B  the split kernel at the edge of its LDS: the largest kh the query reports as split at kw = 18 and 33 (KS = 2) and
   kh + 1, which must be the fp32 kernel; kh = 33 at kw = 17 (KS = 1).
C  the Poisson epilogue at one width per KC class: gradient written, accumulated with grad_scale != 1, npred_out given,
   loss only, against `step_oracle`; npred bit-equal to convolution + poisson_fused_kernel (JD_SEP_NO_FUSION=1); the
   clamp's backward mask in the KS = 2 split kernel (a PSF with negative lobes).
D  more tiles than blocks (JD_CONV_BLOCKS_PER_CU=1, tiles > compute units): the software-pipelined second trip of a
   block's tile loop, forward, adjoint and Poisson, both kernels, both stagings.
E  windows the split kernel scales: an all-zero window, one near 1e-20 and one near 1e+20 in one image, per pixel.
F  every image of a launch in turn only 4-byte aligned: the bits of the aligned run.

Float4 staging needs W % 4 == 0 and the window's first column a multiple of 4: kw / 2 (forward) or (kw - 1) / 2
(adjoint) a multiple of 4.  No width of the classes KC = 20, 28, 36, 44 (kw = 2-5, 10-13, 18-21, 26-29) has the
former, so their forward and Poisson launches always stage scalars; their float4 instantiation runs as the adjoint of
kw = 2, 10, 18, 26.  Every other class runs float4 in both directions (kw = 1, 9, 17, 25, 33).  Part D's 5 x 7 PSF
(kw / 2 = 3) stages scalars at either image width, so it runs a 5 x 9 PSF too, which stages float4 at W % 4 == 0.
(A tile count that is no multiple of 8 leaves work items beyond the grid, which blocks take on a second trip: part E's
22 tiles reach the pipelined loop as well, part A's 4 do not.)

Bounds: positive images 2e-6 (relative L-inf, the project's figure for this kernel); the Poisson step 1e-5 on npred and
gradient, 5e-6 on the loss; the adjoint of a signed image bound() = 4 x the float32 oracle's own distance from float64,
floor 2e-6; part E 3e-6 of each pixel's own value.  The float32 oracle is the same direct sum as the float64 one
(torch conv2d on the CPU) in float32.

Largest figures on an MI355X, kernel | float32 oracle, both against float64 (relative L-inf; E: per pixel):
  A fp32 : fwd 1.59e-06 | 1.42e-06, adj 1.23e-06 | 1.16e-06, acc 9.93e-07 | 9.32e-07; without the scale image fwd 1.68e-06 | 1.30e-06,
           adj 1.21e-06 | 1.21e-06, acc 9.37e-07 | 9.26e-07
  A split: fwd 5.57e-07 | 1.11e-06, adj 3.59e-07 | 7.94e-07, acc 3.13e-07 | 7.29e-07; without fwd 5.10e-07 | 9.61e-07,
           adj 3.53e-07 | 8.75e-07, acc 3.26e-07 | 7.89e-07
  B fp32 : fwd 1.52e-06 | 1.47e-06, adj 1.18e-06 | 5.56e-07, acc 1.11e-06 | 5.23e-07   (kh = 30 at kw = 18 and 33: one past the split kernel)
  B split: fwd 6.02e-07 | 1.33e-06, adj 4.20e-07 | 1.14e-06, acc 2.96e-07 | 7.81e-07   (kh = 29 at kw = 18 and 33, kh = 33 at kw = 17)
  C fp32 : loss 1.40e-07 | 2.40e-08, npred 1.16e-06 | 1.25e-06, grad 1.05e-06 | 9.72e-07, grad accumulated 1.02e-07 | 8.26e-08
  C split: loss 1.40e-07 | 2.40e-08, npred 3.67e-07 | 7.83e-07, grad 3.18e-07 | 6.87e-07, grad accumulated 6.72e-08 | 5.99e-08
  D fp32 : fwd 3.08e-07 | 3.23e-07, adj 3.04e-07 | 3.27e-07, acc 2.84e-07 | 3.16e-07, loss 1.25e-07 | 6.12e-09, npred 3.42e-07 | 2.72e-07,
           grad 3.43e-07 | 3.74e-07
  D split: fwd 1.74e-07 | 3.29e-07, adj 1.84e-07 | 2.53e-07, acc 1.74e-07 | 2.14e-07, loss 1.25e-07 | 6.12e-09, npred 1.93e-07 | 2.72e-07,
           grad 2.00e-07 | 3.74e-07
  E fp32 : fwd 1.05e-06 | 9.84e-07, adj 9.20e-07 | 1.00e-06     E split: fwd 3.72e-07 | 9.59e-07, adj 3.99e-07 | 9.74e-07
  F      : every image of every launch, both kernels: the aligned run's bits
(The fp32 kernel is one fmaf chain over the kh x kw taps, like the float32 oracle: at 33 x 33 both are 1.5e-6 from float64.
The split kernel comes out at a third to a half of that.  The loss: a thread's sixteen terms are summed in float32 before
they join the float64 sum.)  The module's 201 cases take 5.8 s of a GPU suite of 203 s.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_oracle
from prior_cases import bound, rel_linf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
POSITIVE, FLOOR, PER_PIXEL = 2e-6, 2e-6, 3e-6  # forward of a positive image | floor of bound() | part E
NPRED, GRAD, LOSS = 1e-5, 1e-5, 5e-6
KERNELS = ("fp32", "split")
WORST = {}  # (part, kernel, quantity) -> (largest error, the float32 oracle's at that case)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    parts = sorted({(part, kernel) for part, kernel, _ in WORST})
    for part, kernel in parts:
        row = ", ".join(f"{q} {e:.2e} | {o:.2e}" for (p, k, q), (e, o) in WORST.items() if (p, k) == (part, kernel))
        print(f"\n  {part} {kernel:5s}: {row}")


def fp32_kc(kw):
    return (15 + kw + 3) // 4 * 4


def split_kc(kw):
    return 32 if kw <= 17 else 64


def dev(array):
    return None if array is None else torch.tensor(np.ascontiguousarray(array, dtype=np.float32), device=DEV)


def held(array, offset=False):
    """`array` in a fresh device allocation, or (`offset`) as a view one float into an allocation: 4-byte aligned."""
    src = torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32))
    buf = torch.empty(src.numel() + int(offset), device=DEV)
    view = buf[int(offset):].reshape(src.shape)
    view.copy_(src)
    assert view.data_ptr() % 16 == (4 if offset else 0) and view.is_contiguous()
    return view


def uniform_psf(rs, kh, kw):
    """Every tap of comparable weight: a wrong or a missing one shows at about 1 / (kh kw)."""
    psf = rs.uniform(size=(kh, kw))
    return (psf / psf.sum()).astype(np.float32)


def corr_same(g, psf):
    """out[y, x] = sum_ab g[y - oy + a, x - ox + b] psf[a, b], zeros outside: the transpose of `step_oracle.conv_same`
    written out (g in a zero frame of (oy, kh - 1 - oy) rows and (ox, kw - 1 - ox) columns, then a valid correlation)."""
    kh, kw = psf.shape
    oy, ox = (kh - 1) // 2, (kw - 1) // 2
    return F.conv2d(F.pad(g[None, None], (ox, kw - 1 - ox, oy, kh - 1 - oy)), psf[None, None])[0, 0]


def open_plan(H, W, kh, kw, kernel, jd_option):
    """A direct plan with the fp32 kernel asked for (`kernel` = "fp32") or left to the default, and what it reports; the
    staging bits are asserted against the shape rule here, KC and split by the caller."""
    from jolideco_amd.ops import ConvPlan

    jd_option("JD_DIRECT_FP32", "1" if kernel == "fp32" else None)
    plan = ConvPlan(H, W, kh, kw, DEV, method="direct")
    assert plan.method == "direct"
    route = plan.direct_kernel()
    assert route["vec_fwd"] == (W % 4 == 0 and (kw // 2) % 4 == 0), route          # first window column: -(kw / 2)
    assert route["vec_adj"] == (W % 4 == 0 and ((kw - 1) // 2) % 4 == 0), route    # first window column: -((kw - 1) / 2)
    if kernel == "fp32":
        assert not route["split"] and route["KC"] == fp32_kc(kw), route
    else:
        assert route["KC"] == (split_kc(kw) if route["split"] else fp32_kc(kw)), route
    return plan, route


class Checks:
    """Collects the comparisons of one case: prints every figure, keeps the largest per part and kernel, fails at the end."""

    def __init__(self, part, kernel, label):
        self.part, self.kernel, self.label, self.failures = part, kernel, label, []

    def record(self, quantity, err, own, limit):
        key = (self.part, self.kernel, quantity)
        if key not in WORST or err > WORST[key][0]:
            WORST[key] = (err, own)
        print(f"{self.label} {quantity}: {err:.3e} | {own:.3e} (limit {limit:.1e})")
        if not err < limit:
            self.failures.append(f"{quantity}: {err:.3e} >= {limit:.1e} (float32 oracle {own:.3e})")

    def image(self, quantity, got, ref64, ref32, limit=None):
        """Relative L-inf against float64; `limit` None: bound() of the float32 oracle's own error."""
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        assert np.isfinite(got).all(), f"{self.label} {quantity}: not finite"
        own = rel_linf(ref32, ref64)
        self.record(quantity, rel_linf(got, ref64), own, bound(own, FLOOR) if limit is None else limit)

    def scalar(self, quantity, got, ref64, ref32, limit):
        self.record(quantity, abs(float(got) - ref64) / abs(ref64), abs(ref32 - ref64) / abs(ref64), limit)

    def per_pixel(self, quantity, got, ref64, ref32, limit):
        """Every pixel relative to its own float64 value; exactly zero where that is zero."""
        got = got.cpu().numpy().astype(np.float64)
        live = ref64 != 0
        assert live.any() and np.isfinite(got).all()
        assert np.all(got[~live] == 0), f"{self.label} {quantity}: {np.count_nonzero(got[~live])} pixels of an all-zero footprint are not 0"
        local = lambda a: float(np.max(np.abs(a[live] - ref64[live]) / np.abs(ref64[live])))  # noqa: E731
        self.record(quantity, local(got), local(ref32.astype(np.float64)), limit)

    def done(self):
        assert not self.failures, f"{self.label}: " + "; ".join(self.failures)


# ------------------------------------------------------------------------------------------------------------------
# convolution and adjoint: inputs, oracles (computed once per geometry, shared by both kernels), the comparison
# ------------------------------------------------------------------------------------------------------------------
def conv_oracles(image, scale, psf, g, acc0, with_unscaled=True):
    """fwd / adj / acc (and their *_ns twins without the scale image) in float64 ("64") and float32 ("32")."""
    out = {}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        c = lambda a: torch.tensor(a).to(dtype)  # noqa: E731  (float32 inputs: exact in either)
        out["fwd" + tag] = step_oracle.conv_same(c(image) * c(scale), c(psf), "direct").numpy()
        adj = corr_same(c(g), c(psf))
        out["adj" + tag] = (adj * c(scale)).numpy()
        out["acc" + tag] = (c(acc0) + adj * c(scale)).numpy()
        if with_unscaled:
            out["fwd_ns" + tag] = step_oracle.conv_same(c(image), c(psf), "direct").numpy()
            out["adj_ns" + tag] = adj.numpy()
            out["acc_ns" + tag] = (c(acc0) + adj).numpy()
    return out


@functools.lru_cache(maxsize=None)
def conv_case(H, W, kh, kw, with_unscaled=True):
    """Positive image, exposure in (0.5, 1.5), a general PSF of comparable taps, a signed upstream gradient and a non-zero
    image to accumulate into."""
    rs = np.random.RandomState(100000 + 1000 * kh + 10 * kw + W % 7)
    case = {
        "image": (0.05 + rs.gamma(2.0, size=(H, W))).astype(np.float32),
        "scale": rs.uniform(0.5, 1.5, size=(H, W)).astype(np.float32),
        "psf": uniform_psf(rs, kh, kw),
        "g": rs.normal(size=(H, W)).astype(np.float32),
        "acc0": (rs.normal(size=(H, W)) / np.sqrt(kh * kw)).astype(np.float32),  # (the size of the adjoint of `g`)
    }
    case.update(conv_oracles(case["image"], case["scale"], case["psf"], case["g"], case["acc0"], with_unscaled))
    return case


def check_conv(plan, case, checks, with_unscaled=True):
    """Forward and adjoint of `plan` on the inputs of `case` against its oracles."""
    shape = case["image"].shape
    khat = plan.psf_spectrum(dev(case["psf"]))
    image, g = dev(case["image"]), dev(case["g"])
    for suffix, scale in (("", dev(case["scale"])), ("_ns", None)) if with_unscaled else (("", dev(case["scale"])),):
        fwd = plan.conv_same(image, scale, khat)
        adj = plan.conv_same_adjoint(g, scale, khat, grad_image=torch.full(shape, NAN, device=DEV))
        acc = plan.conv_same_adjoint(g, scale, khat, grad_image=dev(case["acc0"]), accumulate=True)
        torch.cuda.synchronize()
        checks.image("fwd" + suffix, fwd, case["fwd" + suffix + "64"], case["fwd" + suffix + "32"], POSITIVE)
        checks.image("adj" + suffix, adj, case["adj" + suffix + "64"], case["adj" + suffix + "32"])
        checks.image("acc" + suffix, acc, case["acc" + suffix + "64"], case["acc" + suffix + "32"])


# ------------------------------------------------------------------------------------------------------------------
# A: the width classes
# ------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 5, 6, 9, 10, 13, 14, 17, 18, 21, 22, 25, 26, 29, 30, 33)  # first and last width of every KC class
HEIGHTS = ((1, 33), (2, 9), (9, 2), (33, 1))  # two of {1, 2, 9, 33} per width (the row loop pairs rows: odd and even)
SHAPES = {"float4": (70, 76), "scalar": (70, 75)}  # 2 x 2 tiles, ragged last row and column


def width_cases():
    return [pytest.param(kh, kw, kernel, staging, id=f"{kh}x{kw}-{kernel}-{staging}")
            for i, kw in enumerate(WIDTHS) for kh in HEIGHTS[i % 4] for kernel in KERNELS for staging in SHAPES]


@pytest.mark.parametrize("kh,kw,kernel,staging", width_cases())
def test_every_width_class_against_float64(kh, kw, kernel, staging, jd_option):
    H, W = SHAPES[staging]
    plan, route = open_plan(H, W, kh, kw, kernel, jd_option)
    try:
        if kernel == "split" and not route["split"]:
            # the planes and the table of the tallest PSFs do not fit beside KS = 2: this plan runs the fp32 kernel, which
            # the "fp32" case of this geometry checks
            assert kw >= 18 and kh == 33, route
            return
        checks = Checks("A", kernel, f"A {kh}x{kw} {kernel} {staging}")
        check_conv(plan, conv_case(H, W, kh, kw), checks)
        checks.done()
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# B: the split kernel's LDS boundary
# ------------------------------------------------------------------------------------------------------------------
def tallest_split(W, kw, jd_option):
    """Largest kh at which a plan of this width reports the split kernel."""
    for kh in range(33, 0, -1):
        plan, route = open_plan(70, W, kh, kw, "split", jd_option)
        plan.close()
        if route["split"]:
            return kh
    return 0


@pytest.mark.parametrize("staging", list(SHAPES))
@pytest.mark.parametrize("kw", [17, 18, 33])
def test_split_kernel_at_the_edge_of_its_lds(kw, staging, jd_option):
    H, W = SHAPES[staging]
    top = tallest_split(W, kw, jd_option)
    if kw == 17:
        assert top == 33  # KS = 1: every height fits
    else:
        assert 1 <= top < 33  # KS = 2: the tallest do not
    for kh in (top, top + 1) if top < 33 else (top,):
        plan, route = open_plan(H, W, kh, kw, "split", jd_option)
        try:
            assert route["split"] == (kh == top) and route["KC"] == (split_kc(kw) if kh == top else fp32_kc(kw)), route
            checks = Checks("B", "split" if kh == top else "fp32", f"B {kh}x{kw} {staging} {'split' if kh == top else 'fp32 (one past)'}")
            check_conv(plan, conv_case(H, W, kh, kw), checks)
            checks.done()
        finally:
            plan.close()


# ------------------------------------------------------------------------------------------------------------------
# C: the Poisson epilogue
# ------------------------------------------------------------------------------------------------------------------
def lobed_psf(rs, kh, kw):
    """The PSF of test_poisson_epilogue_of_the_convolution_matches_the_two_kernel_path at another size: not separable,
    negative between the sources."""
    gy = np.exp(-0.5 * ((np.arange(kh) - (kh - 1) / 2) / (kh / 8.0)) ** 2)
    gx = np.exp(-0.5 * ((np.arange(kw) - (kw - 1) / 2) / (kw / 8.0)) ** 2)
    psf = np.outer(gy, gx) * (1.0 + 0.3 * rs.uniform(-1, 1, size=(kh, kw))) - 0.02
    return (psf / psf.sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def poisson_case(H, W, kh, kw, lobes=False):
    rs = np.random.RandomState(200000 + 1000 * kh + 10 * kw + W % 7)
    case = {
        "flux": (0.1 + rs.gamma(3.0, size=(H, W))).astype(np.float32),
        "exposure": rs.uniform(0.5, 1.5, size=(H, W)).astype(np.float32),
        "psf": lobed_psf(rs, kh, kw) if lobes else uniform_psf(rs, kh, kw),
        "background": rs.uniform(0.2, 1.0, size=(H, W)).astype(np.float32),
        "counts": rs.poisson(3.0, size=(H, W)).astype(np.float32),
        "acc0": (1e-4 * rs.normal(size=(H, W))).astype(np.float32),  # (the size of the gradient: d loss / d flux ~ 1 / (H W))
    }
    if lobes:  # sparse sources: the negative lobes win between them
        case["flux"] = case["flux"] * (rs.uniform(size=(H, W)) < 0.01)
    args = (case["flux"], case["exposure"], case["psf"], case["background"], case["counts"], 1)
    case["ref64"] = step_oracle.step_oracle(*args, conv="direct")
    case["ref32"] = step_oracle.step_oracle(*args, dtype=torch.float32, conv="direct")
    case["stirling"] = step_oracle.stirling_mean(case["counts"])
    return case


def poisson_runs(plan, case):
    """The four forms of the step: gradient written | accumulated with grad_scale = 0.5 | npred_out given | loss only."""
    shape = case["flux"].shape
    khat = plan.psf_spectrum(dev(case["psf"]))
    flux, exposure, background, counts = (dev(case[k]) for k in ("flux", "exposure", "background", "counts"))
    step = lambda loss, **kw: plan.npred_poisson_fwd_bwd([flux], [exposure], [khat], background, counts, case["stirling"],  # noqa: E731
                                                         loss, **kw)
    losses = [torch.full((1,), NAN, device=DEV) for _ in range(4)]
    grad, acc, grad_n = torch.full(shape, NAN, device=DEV), dev(case["acc0"]), torch.full(shape, NAN, device=DEV)
    npred = torch.full(shape, NAN, device=DEV)
    step(losses[0], grads=[grad])
    step(losses[1], grads=[acc], accumulate=True, grad_scale=0.5)
    step(losses[2], grads=[grad_n], npred_out=npred)
    step(losses[3])
    torch.cuda.synchronize()
    return {"losses": [float(v) for v in losses], "grad": grad.cpu().numpy(), "acc": acc.cpu().numpy(),
            "grad_n": grad_n.cpu().numpy(), "npred": npred.cpu().numpy()}


def launches_of_a_loss(plan, case):
    """(direct_conv_kernel launches, Poisson launches) the library's timers count for one loss-only step."""
    from jolideco_amd import _hip

    khat = plan.psf_spectrum(dev(case["psf"]))
    tensors = [dev(case[k]) for k in ("flux", "exposure", "background", "counts")]
    loss = torch.zeros(1, device=DEV)
    _hip.profile_enable(64)
    plan.npred_poisson_fwd_bwd([tensors[0]], [tensors[1]], [khat], tensors[2], tensors[3], case["stirling"], loss)
    stats = _hip.profile_read()
    return stats["direct_conv"][1], stats["poisson_fused"][1]


def check_poisson(got, case, checks, gradient=True):
    ref64, ref32 = case["ref64"], case["ref32"]
    for i, loss in enumerate(got["losses"]):
        checks.scalar(f"loss{i}", loss, ref64["loss"], ref32["loss"], LOSS)
    checks.image("npred", got["npred"], ref64["npred"], ref32["npred"], NPRED)
    if gradient:
        checks.image("grad", got["grad"], ref64["grad_flux"], ref32["grad_flux"], GRAD)
        checks.image("grad_n", got["grad_n"], ref64["grad_flux"], ref32["grad_flux"], GRAD)
        acc0 = case["acc0"].astype(np.float64)
        checks.image("grad_acc", got["acc"], acc0 + 0.5 * ref64["grad_flux"], (case["acc0"] + np.float32(0.5) * ref32["grad_flux"].astype(np.float32)), GRAD)


POISSON_SIZES = ((9, 1), (2, 5), (33, 9), (1, 13), (9, 17), (2, 21), (33, 25), (1, 29), (9, 33))  # one width per KC class


@pytest.mark.parametrize("staging", list(SHAPES))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kh,kw", POISSON_SIZES)
def test_poisson_epilogue_against_float64(kh, kw, kernel, staging, jd_option):
    H, W = SHAPES[staging]
    plan, route = open_plan(H, W, kh, kw, kernel, jd_option)
    try:
        if kernel == "split" and not route["split"]:
            assert kw >= 18 and kh == 33, route  # (as in part A)
            return
        case = poisson_case(H, W, kh, kw)
        assert step_oracle.clip_margin(case["ref64"]["pooled"]) >= 1e-3 and case["ref64"]["pooled"][0].min() > 0
        results = {}
        for fusion in ("epilogue", "two-kernel"):
            jd_option("JD_SEP_NO_FUSION", None if fusion == "epilogue" else "1")
            assert launches_of_a_loss(plan, case) == ((0, 1) if fusion == "epilogue" else (1, 1))
            results[fusion] = poisson_runs(plan, case)
            checks = Checks("C", kernel, f"C {kh}x{kw} {kernel} {staging} {fusion}")
            check_poisson(results[fusion], case, checks)
            checks.done()
        assert np.array_equal(results["epilogue"]["npred"], results["two-kernel"]["npred"])  # same arithmetic, same bits
    finally:
        plan.close()


def test_clamp_mask_of_the_two_step_split_kernel(jd_option):
    """Negative lobes, sparse sources: conv < 0 on part of the image, where the clamp passes no gradient -- in the KS = 2
    instantiation of the split kernel (the existing test has it at 17 x 17, KS = 1)."""
    H, W, kh, kw = 97, 152, 25, 25
    plan, route = open_plan(H, W, kh, kw, "split", jd_option)
    try:
        assert route == {"KC": 64, "split": True, "vec_fwd": True, "vec_adj": True}
        case = poisson_case(H, W, kh, kw, lobes=True)
        conv = case["ref64"]["pooled"][0]
        assert 0.05 < (conv < 0).mean() < 0.95
        results = {}
        for fusion in ("epilogue", "two-kernel"):
            jd_option("JD_SEP_NO_FUSION", None if fusion == "epilogue" else "1")
            assert launches_of_a_loss(plan, case) == ((0, 1) if fusion == "epilogue" else (1, 1))
            results[fusion] = poisson_runs(plan, case)
            checks = Checks("C", "split", f"C lobes {kh}x{kw} {fusion}")
            check_poisson(results[fusion], case, checks, gradient=False)  # (the clamp is a kink: a pixel at it may go either way)
            checks.done()
        a, b = results["epilogue"], results["two-kernel"]
        assert np.array_equal(a["npred"], b["npred"])
        # the mask itself, away from the kink: clamped exactly where the float64 convolution is negative
        clear = np.abs(conv) > 1e-4 * np.abs(conv).max()
        assert clear.mean() > 0.9 and np.array_equal((a["npred"] == case["background"])[clear], (conv < 0)[clear])
        for key in ("grad", "grad_n", "acc"):  # the same g, the same adjoint kernel
            assert rel_linf(a[key], b[key]) < 1e-6, key
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# D: more tiles than blocks
# ------------------------------------------------------------------------------------------------------------------
def pipelined_shape(staging):
    """Smallest square of tiles that outnumbers the compute units (one block each), ragged last tile row and column: on
    an MI355X (256) 17 x 17 = 289 tiles -- 33 blocks walk a second tile, and 289 is no multiple of 8, so the XCD-ordered
    `tile_of` has holes."""
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    side = int(np.floor(np.sqrt(n_cu))) + 1
    H, W = 64 * (side - 1) + 6, 64 * (side - 1) + (4 if staging == "float4" else 3)
    tiles = ((H + 63) // 64) * ((W + 63) // 64)
    assert n_cu < tiles < 2 * n_cu, (n_cu, tiles)
    return H, W


@pytest.mark.parametrize("staging", list(SHAPES))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kh,kw", [(5, 7), (5, 9)])
def test_blocks_that_walk_a_second_tile(kh, kw, kernel, staging, jd_option):
    jd_option("JD_CONV_BLOCKS_PER_CU", "1")
    H, W = pipelined_shape(staging)
    plan, route = open_plan(H, W, kh, kw, kernel, jd_option)
    try:
        assert route["split"] == (kernel == "split")
        assert route["vec_fwd"] == route["vec_adj"] == (staging == "float4" and kw == 9), route
        checks = Checks("D", kernel, f"D {H}x{W} {kh}x{kw} {kernel} {staging}")
        check_conv(plan, conv_case(H, W, kh, kw, False), checks, with_unscaled=False)
        case = poisson_case(H, W, kh, kw)
        assert step_oracle.clip_margin(case["ref64"]["pooled"]) >= 1e-3
        assert launches_of_a_loss(plan, case) == (0, 1)
        check_poisson(poisson_runs(plan, case), case, checks)
        checks.done()
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# E: windows the split kernel scales
# ------------------------------------------------------------------------------------------------------------------
# tile columns of 64: ordinary | gap gap gap | 1e-20 | gap gap | 1e+20 | gap gap | ordinary (ragged).  A window reaches less
# than one tile beyond its own, so with two gap columns between them no window holds values of two magnitudes (the split
# kernel scales a window by ONE power of two: a pixel 1e-20 of its window's brightest has no bits left, by design), and
# the window of the middle of the three gap columns is entirely zero.
E_COLUMNS = (1.0, 0.0, 0.0, 0.0, 1e-20, 0.0, 0.0, 1e20, 0.0, 0.0, 1.0)
E_ZERO_TILE = 2


@functools.lru_cache(maxsize=None)
def scaled_case(W, kh, kw):
    H = 70
    rs = np.random.RandomState(300000 + 10 * kw + W % 7)
    magnitude = np.repeat(np.asarray(E_COLUMNS), 64)[:W]
    image = (rs.uniform(0.5, 2.0, size=(H, W)) * np.where(magnitude > 0, magnitude, 1.0)).astype(np.float32)
    exposure = (rs.uniform(0.5, 1.5, size=(H, W)) * (magnitude > 0)).astype(np.float32)  # the gaps are exposure gaps
    u = image * exposure  # (float32: what the adjoint gets as its upstream image)
    x0 = 64 * E_ZERO_TILE
    assert np.all(u[:, x0 - 64 : x0 + 128] == 0) and np.all(u[:, : x0 - 64] > 0)
    case = {"image": image, "scale": exposure, "psf": uniform_psf(rs, kh, kw), "g": u,
            "scale_adj": rs.uniform(0.5, 1.5, size=(H, W)).astype(np.float32)}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        c = lambda a: torch.tensor(a).to(dtype)  # noqa: E731
        case["fwd" + tag] = step_oracle.conv_same(c(image) * c(exposure), c(case["psf"]), "direct").numpy()
        case["adj" + tag] = (corr_same(c(u), c(case["psf"])) * c(case["scale_adj"])).numpy()
    return case


@pytest.mark.parametrize("staging,W", [("float4", 644), ("scalar", 643)])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kh,kw", [(9, 9), (9, 25)])
def test_windows_of_zero_of_1e_minus_20_and_of_1e_plus_20(kh, kw, kernel, staging, W, jd_option):
    plan, route = open_plan(70, W, kh, kw, kernel, jd_option)
    try:
        assert route["split"] == (kernel == "split") and route["vec_fwd"] == route["vec_adj"] == (staging == "float4"), route
        case = scaled_case(W, kh, kw)
        khat = plan.psf_spectrum(dev(case["psf"]))
        fwd = plan.conv_same(dev(case["image"]), dev(case["scale"]), khat)
        adj = plan.conv_same_adjoint(dev(case["g"]), dev(case["scale_adj"]), khat, grad_image=torch.full((70, W), NAN, device=DEV))
        torch.cuda.synchronize()
        tile = slice(64 * E_ZERO_TILE, 64 * E_ZERO_TILE + 64)
        assert np.all(case["fwd64"][:, tile] == 0) and np.all(case["adj64"][:, tile] == 0)
        for name, span in (("1e-20", slice(256, 320)), ("1e+20", slice(448, 512))):  # the oracle sees the three magnitudes
            ratio = case["fwd64"][:, span].max() / float(name)
            assert 0.1 < ratio < 10, (name, ratio)
        checks = Checks("E", kernel, f"E {kh}x{kw} {kernel} {staging}")
        checks.per_pixel("fwd", fwd, case["fwd64"], case["fwd32"], PER_PIXEL)
        checks.per_pixel("adj", adj, case["adj64"], case["adj32"], PER_PIXEL)
        checks.done()
        assert float(fwd[:, tile].abs().max()) == 0 and float(adj[:, tile].abs().max()) == 0
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------
# F: images that are only 4-byte aligned
# ------------------------------------------------------------------------------------------------------------------
F_IMAGES = {"forward": ("image", "scale", "out"), "adjoint": ("g", "scale", "acc"),
            "poisson": ("flux", "exposure", "background", "counts", "npred", "grad")}


def run_held(plan, op, khat, arrays, offset):
    """One launch of `op` with the image named `offset` (or none) one float into its allocation; the images it wrote."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, stream_ptr

    t = {name: held(arrays[name], name == offset) for name in F_IMAGES[op]}
    if op == "forward":
        check(_hip.lib().jd_conv_same(plan._handle, ptr(t["image"]), ptr(t["scale"]), ptr(khat), ptr(t["out"]), stream_ptr(DEV)))
        wrote = ("out",)
    elif op == "adjoint":
        plan.conv_same_adjoint(t["g"], t["scale"], khat, grad_image=t["acc"], accumulate=True)
        wrote = ("acc",)
    else:
        loss = torch.full((1,), NAN, device=DEV)
        plan.npred_poisson_fwd_bwd([t["flux"]], [t["exposure"]], [khat], t["background"], t["counts"], arrays["stirling"], loss,
                                   grads=[t["grad"]], accumulate=True, grad_scale=0.5, npred_out=t["npred"])
        t["loss"], wrote = loss, ("npred", "grad", "loss")
    torch.cuda.synchronize()
    return {name: t[name].clone() for name in wrote}


@pytest.mark.parametrize("op", list(F_IMAGES))
@pytest.mark.parametrize("kernel", KERNELS)
def test_four_byte_aligned_images_give_the_aligned_bits(kernel, op, jd_option):
    """A fit's second flux component has its gradient image in a slice of one flat buffer: 4-byte aligned when the first
    component's pixel count is no multiple of 4.  Staging and epilogue move float4 only between 16-byte aligned images."""
    H, W, kh, kw = 70, 76, 9, 9
    plan, route = open_plan(H, W, kh, kw, kernel, jd_option)
    try:
        assert route["split"] == (kernel == "split") and route["vec_fwd"] and route["vec_adj"], route
        conv, poisson = conv_case(H, W, kh, kw), poisson_case(H, W, kh, kw)
        arrays = {"image": conv["image"], "scale": conv["scale"], "out": np.full((H, W), NAN), "g": conv["g"], "acc": conv["acc0"],
                  "flux": poisson["flux"], "exposure": poisson["exposure"], "background": poisson["background"],
                  "counts": poisson["counts"], "npred": np.full((H, W), NAN), "grad": poisson["acc0"], "stirling": poisson["stirling"]}
        khat = plan.psf_spectrum(dev(conv["psf"] if op != "poisson" else poisson["psf"]))
        want = run_held(plan, op, khat, arrays, None)
        checks = Checks("F", kernel, f"F {op} {kernel} aligned")  # the aligned run itself is right
        if op == "forward":
            checks.image("fwd", want["out"], conv["fwd64"], conv["fwd32"], POSITIVE)
        elif op == "adjoint":
            checks.image("acc", want["acc"], conv["acc64"], conv["acc32"])
        else:
            checks.image("npred", want["npred"], poisson["ref64"]["npred"], poisson["ref32"]["npred"], NPRED)
            checks.scalar("loss", want["loss"], poisson["ref64"]["loss"], poisson["ref32"]["loss"], LOSS)
        checks.done()
        for name in F_IMAGES[op]:
            got = run_held(plan, op, khat, arrays, name)
            for key, value in want.items():
                assert bool(torch.isfinite(value).all())
                assert torch.equal(got[key], value), (
                    f"{op}, {kernel}, `{name}` 4-byte aligned: {key} differs in {int((got[key] != value).sum())} of {value.numel()} pixels")
    finally:
        plan.close()

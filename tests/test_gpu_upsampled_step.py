"""The (calibrated, up-sampled) likelihood step -- jd_npred_poisson_calibrated_fwd_bwd and
jd_npred_poisson_calibrated_batch_fwd_bwd -- called on `ConvPlan` directly, against the float64 oracle of
tests/step_oracle.py: every up-sampling factor of the fused launches x every row schedule x pooled column I/O on / off (A),
the shift geometry (B), the three tilings of the transposed shift (C) and the generic route (D).  Every case first asks
`ConvPlan.step_route` (jd_conv_plan_step_route) which kernels it is about to run and asserts that they are the ones it means.

Inputs (positive everywhere, so that the clip of the pooled convolution is never near its kink; `ref` asserts it):
flux = 0.5 + gamma(2), exposure in (0.5, 1.5), psf = 0.2 + uniform^3 normalised, background in (0.5, 1), counts Poisson(6).

Bounds (tests/test_gpu_baseline_parity.py `_check_c6_shaped_step`): loss rtol 5e-6, flux gradient relative L-inf < 1e-5,
shift gradient rtol 1e-4 + 2e-5 max|ref|, norm gradient rtol 2e-5.  A shift gradient (a cancelling sum) that misses its bound
is allowed 4 x the distance of the SAME oracle run in float32 from float64 (floor 1e-6 max|ref|); the measured errors are in
profiles/step_matrix/README.md."""
import functools

import numpy as np
import pytest
import torch

import step_oracle
from conftest import rel_linf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# inputs, oracle, device calls
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(Hd, Wd, k, U, n_datasets=1, psf_kind="general"):
    """(flux, datasets) of a counts grid (Hd, Wd) with a k x k PSF in counts pixels: flux-grid arrays U times that size."""
    rs = np.random.RandomState((Hd * 7919 + Wd * 104729 + k * 31 + U * 7) % (2**31))
    H, W = U * Hd, U * Wd
    flux = (0.5 + rs.gamma(2.0, size=(H, W))).astype(np.float32)
    datasets = []
    for d in range(n_datasets):
        if psf_kind == "gauss":  # rank 1: what a separable plan takes
            t = np.arange(U * k) - (U * k - 1) / 2
            g = np.exp(-0.5 * (t / (0.24 * U * k + 0.05 * d)) ** 2)
            psf = np.outer(g, g)
        else:
            psf = 0.2 + rs.uniform(size=(U * k, U * k)) ** 3
        datasets.append({
            "exposure": rs.uniform(0.5, 1.5, size=(H, W)).astype(np.float32),
            "psf": (psf / psf.sum()).astype(np.float32),
            "background": rs.uniform(0.5, 1.0, size=(Hd, Wd)).astype(np.float32),
            "counts": rs.poisson(6.0, size=(Hd, Wd)).astype(np.float32),
        })
    return flux, datasets


def _oracle(key, d, shift, log_norm, dtype):
    flux, datasets = inputs(*key)
    ds = datasets[d]
    out = step_oracle.step_oracle(flux, ds["exposure"], ds["psf"], ds["background"], ds["counts"], key[3], shift=shift,
                                  log_norm=log_norm, dtype=dtype)
    if dtype == torch.float64:
        margin = step_oracle.clip_margin(out["pooled"])
        assert margin >= 1e-3, f"a pooled convolution at {margin:.1e} of the maximum: too close to the clip"
    del out["pooled"]
    return out


_cached_oracle = functools.lru_cache(maxsize=None)(_oracle)


def ref(key, d=0, shift=None, log_norm=None, dtype=torch.float64):
    """The oracle of dataset d of `inputs(*key)`, computed once per case (images beyond a megapixel are not kept)."""
    big = key[0] * key[1] * key[3] ** 2 > 1 << 20
    return (_oracle if big else _cached_oracle)(key, d, shift, log_norm, dtype)


class Device:
    """The arrays of `inputs(*key)` on the GPU with a plan and one operator per dataset."""

    def __init__(self, key, method="fft"):
        from jolideco_amd.ops import ConvPlan

        flux, datasets = inputs(*key)
        Hd, Wd, k, U = key[:4]
        self.key, self.U = key, U
        self.plan = ConvPlan(U * Hd, U * Wd, U * k, U * k, DEV, method=method)
        self.flux = torch.from_numpy(flux).to(DEV)
        self.ds = []
        for ds in datasets:
            t = {name: torch.from_numpy(a).to(DEV) for name, a in ds.items()}
            t["khat"] = self.plan.psf_spectrum(t["psf"])
            t["stirling"] = step_oracle.stirling_mean(ds["counts"])
            self.ds.append(t)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.plan.close()
        return False

    def calibration(self, shift, log_norm):
        """(shift_xy, log_norm, grad_shift_xy, grad_log_norm) device tensors (None where there is none); the gradients
        start as NaN: the library must overwrite them."""
        if shift is None and log_norm is None:
            return None
        st = None if shift is None else torch.tensor(shift, dtype=torch.float32, device=DEV)
        nt = None if log_norm is None else torch.tensor([log_norm], dtype=torch.float32, device=DEV)
        return (st, nt, None if st is None else torch.full((2,), NAN, device=DEV), None if nt is None else torch.full((1,), NAN, device=DEV))

    def grad_image(self, fill):
        return torch.full_like(self.flux, fill)

    def single(self, d=0, shift=None, log_norm=None, grad=None, accumulate=False, grad_scale=1.0, npred_out=None):
        """One dataset through `npred_poisson_fwd_bwd`; without `grad` the gradient image starts as NaN."""
        ds, cal = self.ds[d], self.calibration(shift, log_norm)
        loss = torch.full((1,), NAN, device=DEV)
        grad = self.grad_image(NAN) if grad is None else grad
        self.plan.npred_poisson_fwd_bwd([self.flux], [ds["exposure"]], [ds["khat"]], ds["background"], ds["counts"], ds["stirling"],
                                        loss, grads=[grad], accumulate=accumulate, grad_scale=grad_scale, npred_out=npred_out,
                                        upsampling=self.U, calibration=cal)
        torch.cuda.synchronize()
        return {"loss": [loss], "grad": grad, "cal": [cal]}

    def loop(self, cals, fill=None, grad_scale=1.0):
        """The per-dataset calls a batched step stands for: `accumulate` from the second dataset on (from the first when
        the gradient image is pre-filled with `fill`)."""
        grad = self.grad_image(NAN if fill is None else fill)
        out = {"loss": [], "grad": grad, "cal": []}
        for d, (shift, log_norm) in enumerate(cals):
            one = self.single(d, shift, log_norm, grad=grad, accumulate=fill is not None or d > 0, grad_scale=grad_scale)
            out["loss"] += one["loss"]
            out["cal"] += one["cal"]
        return out

    def batch(self, cals, fill=None, grad_scale=1.0):
        """All datasets through `npred_poisson_calibrated_batch_fwd_bwd`."""
        grad = self.grad_image(NAN if fill is None else fill)
        losses = [torch.full((1,), NAN, device=DEV) for _ in cals]
        tuples = [self.calibration(shift, log_norm) for shift, log_norm in cals]
        col = lambda name: [ds[name] for ds in self.ds[: len(cals)]]  # noqa: E731
        self.plan.npred_poisson_calibrated_batch_fwd_bwd(self.flux, col("exposure"), col("khat"), col("background"), col("counts"),
                                                         col("stirling"), losses, tuples, upsampling=self.U, grad=grad,
                                                         accumulate=fill is not None, grad_scale=grad_scale)
        torch.cuda.synchronize()
        return {"loss": losses, "grad": grad, "cal": tuples}


def assert_same_bits(a, b):
    """Every output of two runs, bit for bit."""
    assert torch.equal(a["grad"], b["grad"]) and bool(torch.isfinite(a["grad"]).all())
    for la, lb in zip(a["loss"], b["loss"]):
        assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
    for ca, cb in zip(a["cal"], b["cal"]):
        assert (ca is None) == (cb is None)
        for ta, tb in zip(ca or (), cb or ()):
            assert (ta is None) == (tb is None)
            assert ta is None or (torch.equal(ta, tb) and bool(torch.isfinite(ta).all()))


def check(label, got, key, cals, fill=None, grad_scale=1.0):
    """Losses, flux gradient (= fill + grad_scale * the sum over the datasets), shift and norm gradients (x grad_scale)
    of a run over the datasets `cals` = [(shift | None, log_norm | None), ...] against the float64 oracle."""
    refs = [ref(key, d, shift, log_norm) for d, (shift, log_norm) in enumerate(cals)]
    want = (fill or 0.0) + grad_scale * sum(r["grad_flux"] for r in refs)
    grad = got["grad"].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(grad)), f"{label}: the gradient image was not written everywhere"
    # the gradient's own 1e-5 and, where the call accumulates, one fp32 rounding per dataset of a sum no larger than
    # |fill| + grad_scale * sum_d max|gradient_d|: 2^-24 of that each
    top = np.abs(want - (fill or 0.0)).max()
    rounding = len(cals) * 2.0**-24 * (abs(fill) + grad_scale * sum(np.abs(r["grad_flux"]).max() for r in refs)) if fill else 0.0
    err_grad = np.abs(grad - want).max()
    figures = [f"flux gradient {err_grad / top:.1e}" + (f" (rounding of the sum allows {rounding / top:.1e})" if fill else "")]
    failures = []
    if not err_grad < 1e-5 * top + rounding:
        failures.append(f"flux gradient {err_grad / top:.2e} >= {1e-5 + rounding / top:.2e}")
    for d, ((shift, log_norm), r) in enumerate(zip(cals, refs)):
        loss = float(got["loss"][d])
        err = abs(loss / r["loss"] - 1)
        figures.append(f"loss[{d}] {err:.1e}")
        if not err <= 5e-6:
            failures.append(f"loss[{d}] {loss} against {r['loss']}")
        cal = got["cal"][d]
        if shift is not None:
            gs, want_s = cal[2].cpu().numpy().astype(np.float64), grad_scale * r["grad_shift"]
            top = np.abs(want_s).max()
            err = np.abs(gs - want_s).max() / top
            figures.append(f"shift[{d}] {err:.1e}")
            if not np.all(np.abs(gs - want_s) <= 1e-4 * np.abs(want_s) + 2e-5 * top):
                r32 = ref(key, d, shift, log_norm, dtype=torch.float32)
                own = np.abs(grad_scale * r32["grad_shift"] - want_s).max() / top
                figures.append(f"(float32 oracle {own:.1e})")
                if not err <= max(4 * own, 1e-6):
                    failures.append(f"shift gradient[{d}] {gs} against {want_s}: {err:.2e}, float32 oracle {own:.2e}")
        if log_norm is not None:
            gn, want_n = float(cal[3]), grad_scale * r["grad_log_norm"]
            err = abs(gn / want_n - 1)
            figures.append(f"norm[{d}] {err:.1e}")
            if not err <= 2e-5:
                failures.append(f"norm gradient[{d}] {gn} against {want_n}")
    print(f"STEP-MATRIX {label}: " + ", ".join(figures))
    assert not failures, f"{label}: " + "; ".join(failures)


SHIFT, LOG_NORM = (0.2, -0.15), float(np.log(1.1))
# a batch of three: distinct PSFs, exposures and calibrations; one dataset without a shift, one without a norm
BATCH_CALS = [((0.2, -0.15), float(np.log(1.1))), (None, float(np.log(0.9))), ((-0.35, 0.4), None)]


# ---------------------------------------------------------------------------------------------------------------------
# A. factor x schedule x pooled column I/O
# ---------------------------------------------------------------------------------------------------------------------
def _matrix():
    table = {
        2: {"generic-small": (24, 40, 5), "1152": (24, 560, 5), "2304": (24, 1100, 5), "4608": (24, 2200, 5), "generic-large": (24, 1010, 5)},
        3: {"generic-small": (24, 40, 5), "1152": (24, 380, 5), "2304": (24, 760, 5), "4608": (24, 1500, 5), "generic-large": (24, 560, 5)},
        4: {"generic-small": (24, 40, 5), "1152": (24, 270, 5), "2304": (24, 560, 5), "4608": (24, 1100, 5), "generic-large": (24, 500, 5)},
    }
    cases = []
    for U, shapes in table.items():
        io = U != 3  # (U = 3: Ny = 64 of these shapes is no multiple of 3)
        for sched, shape in shapes.items():
            cases.append((U, shape, sched, io, {}))
        small = shapes["generic-small"]
        cases.append((U, small, "tiny", io, {"JD_FFT_TINY": 1024}))  # one wave per row pair: the shifted load with QB = 1
        cases.append((U, (24, 40, 4), "generic-small", io, {}))  # even PSF size
        if U != 4:
            cases.append((U, (24, 41, 5), "generic-small", io, {}))  # flux width % 4 != 0: ragged rows, scalar shift kernels
            cases.append((U, (24, 41, 5), "tiny", io, {"JD_FFT_TINY": 1024}))
        if U != 3:
            cases.append((U, small, "generic-small", False, {"JD_FFT_POOL_IO": 0}))
            cases.append((U, shapes["2304"], "2304", False, {"JD_FFT_POOL_IO": 0}))
    cases.append((3, (30, 50, 7), "generic-small", True, {}))  # Hh = 45, Ny = 72: pooled I/O at U = 3
    cases.append((3, (30, 50, 7), "generic-small", False, {"JD_FFT_POOL_IO": 0}))
    cases.append((4, (12, 40, 5), "generic-small", False, {}))  # Hh / U = 6 < 3 + 3 + 1 pooled seam rows: I/O off by itself
    return cases


def _case_id(case):
    U, shape, sched, io, options = case
    return f"u{U}-{'x'.join(map(str, shape))}-{sched}-io{int(io)}"


@pytest.mark.parametrize("case", _matrix(), ids=_case_id)
def test_factor_schedule_pooled_io(case, jd_option):
    """One dataset (uncalibrated; calibrated; calibrated accumulating onto a pre-filled gradient with grad_scale 0.5) and a
    batch of three against the oracle, the batch bit for bit against its per-dataset calls (include/jolideco_hip.h:
    jd_npred_poisson_calibrated_batch_fwd_bwd), again with JD_FFT_BATCH=0."""
    U, (Hd, Wd, k), sched, io, options = case
    for name, value in options.items():
        jd_option(name, value)
    key = (Hd, Wd, k, U, 3)
    label = _case_id(case)
    with Device(key) as dev:
        assert dev.plan.native_fft
        vec = 1 if (U * Wd) % 4 == 0 else 0
        route = dev.plan.step_route(U, 1)
        assert (route["rows_fwd"], route["rows_pooled"]) == (sched, sched), route
        assert route["pooled_supported"] and route["pooled_column_io"] == io and route["shift_bwd_rows"] == vec, route
        check(f"{label} uncalibrated", dev.single(0), key, [(None, None)])
        check(f"{label} calibrated", dev.single(0, SHIFT, LOG_NORM), key, [(SHIFT, LOG_NORM)])
        check(f"{label} calibrated accumulate", dev.single(0, SHIFT, LOG_NORM, grad=dev.grad_image(0.5), accumulate=True, grad_scale=0.5),
              key, [(SHIFT, LOG_NORM)], fill=0.5, grad_scale=0.5)
        check(f"{label} uncalibrated accumulate", dev.single(0, grad=dev.grad_image(0.5), accumulate=True, grad_scale=0.5),
              key, [(None, None)], fill=0.5, grad_scale=0.5)
        route = dev.plan.step_route(U, 3)
        want = "tiny" if "JD_FFT_TINY" in options else sched
        assert (route["rows_fwd"], route["rows_pooled"], route["batched"]) == (want, want, 1), route
        batch = dev.batch(BATCH_CALS)
        assert_same_bits(batch, dev.loop(BATCH_CALS))
        check(f"{label} batch of 3", batch, key, BATCH_CALS)
        batch = dev.batch(BATCH_CALS, fill=0.5, grad_scale=0.5)
        assert_same_bits(batch, dev.loop(BATCH_CALS, fill=0.5, grad_scale=0.5))
        check(f"{label} batch of 3 accumulate", batch, key, BATCH_CALS, fill=0.5, grad_scale=0.5)
        uncal = [(None, None)] * 3  # (up-sampling alone goes through the same entry)
        batch = dev.batch(uncal)
        assert_same_bits(batch, dev.loop(uncal))
        check(f"{label} uncalibrated batch of 3", batch, key, uncal)
        jd_option("JD_FFT_BATCH", 0)
        assert dev.plan.step_route(U, 3)["batched"] == 0
        assert_same_bits(dev.batch(BATCH_CALS), dev.loop(BATCH_CALS))


# ---------------------------------------------------------------------------------------------------------------------
# B. shift geometry
# ---------------------------------------------------------------------------------------------------------------------
# in counts pixels: sub-pixel; several pixels; integer after x 2; integer (below the PSF's half width, see the module
# docstring of tests/step_oracle.py and `ref`'s clip guard); windows that leave the image by many pixels
SHIFTS = [(0.2, -0.15), (1.25, -2.5), (1.5, -1.0), (-2.0, 2.0), (2.0, 0.0), (7.5, -9.5), (-17.5, 2.5)]
GEOMETRY = [(2, (24, 40, 5), "generic-small"), (2, (24, 41, 5), "generic-small"), (3, (24, 40, 5), "generic-small"),
            (3, (24, 41, 5), "generic-small"), (4, (24, 40, 5), "generic-small"), (2, (24, 1100, 5), "2304"),
            (2, (24, 2200, 5), "4608")]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate-kernels"])
@pytest.mark.parametrize("U,shape,sched", GEOMETRY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_shift_geometry(U, shape, sched, fused, jd_option):
    """Shifts of several (up-sampled) pixels, exactly integer shifts and shifts that move the whole image out, through the
    fused row load (`fftn_rows_fwd_kernel` + issue_row5) and through the stand-alone `shift_fwd_kernel`
    (JD_SEP_NO_FUSION=1); the transposed shift runs the four-pixel kernel or, where W % 4 != 0, the scalar ones."""
    if not fused:
        jd_option("JD_SEP_NO_FUSION", 1)
    Hd, Wd, k = shape
    key = (Hd, Wd, k, U, 3)
    label = f"u{U}-{'x'.join(map(str, shape))}-{sched}-{'fused' if fused else 'separate'}"
    with Device(key) as dev:
        route = dev.plan.step_route(U, 1)
        assert dev.plan.native_fft and route["rows_fwd"] == sched and route["pooled_supported"], route
        assert route["shift_bwd_rows"] == (1 if (U * Wd) % 4 == 0 else 0), route
        for shift in SHIFTS:
            check(f"{label} shift {shift}", dev.single(0, shift, LOG_NORM), key, [(shift, LOG_NORM)])
        # the whole image moved out: nothing depends on the flux or on the shift any more
        for shift in ((Wd + 3.5, 0.25), (0.3, -(Hd + 1.5))):
            got, r = dev.single(0, shift, LOG_NORM), ref(key, 0, shift, LOG_NORM)
            assert abs(float(got["loss"][0]) / r["loss"] - 1) <= 5e-6
            assert abs(float(got["cal"][0][3]) / r["grad_log_norm"] - 1) <= 2e-5
            assert not np.any(r["grad_flux"]) and not np.any(r["grad_shift"])
            assert int(torch.count_nonzero(got["grad"])) == 0 and bool(torch.isfinite(got["grad"]).all())
            assert int(torch.count_nonzero(got["cal"][0][2])) == 0 and bool(torch.isfinite(got["cal"][0][2]).all())
        # three datasets with shifts of different kinds in one batched transposed-shift launch
        cals = [(SHIFTS[1], LOG_NORM), (SHIFTS[3], None), (SHIFTS[5], LOG_NORM)]
        assert dev.plan.step_route(U, 3)["batched"] == (1 if fused else 0)
        batch = dev.batch(cals)
        assert_same_bits(batch, dev.loop(cals))
        check(f"{label} batch of 3 shifts", batch, key, cals)


# ---------------------------------------------------------------------------------------------------------------------
# C. tilings of the transposed shift
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,rows", [(2051, 2), (4093, 4)])
def test_shift_backward_tiling_separable(H, rows):
    """`shift_bwd4_kernel<2>` / `<4>` at the smallest image that reaches them (W = 1024; the last row group is ragged):
    separable plan, no up-sampling, rank-1 Gaussian 5 x 5 PSF, shift (1.25, -2.5)."""
    key = (H, 1024, 5, 1, 1, "gauss")
    with Device(key, method="separable") as dev:
        route = dev.plan.step_route(1, 1)
        assert dev.plan.method == "separable" and route["shift_bwd_rows"] == rows, route
        check(f"separable {H}x1024 R={rows}", dev.single(0, (1.25, -2.5), None), key, [((1.25, -2.5), None)])


def test_shift_backward_tiling_native_4096_rows():
    """The route of bench.py's c6 at a quarter of its width: flux grid 4096 x 1024 (counts 2048 x 512, k = 5), up-sampling
    x 2 -- 1152-point rows, 2304-point columns, R = 4 -- one calibrated dataset."""
    key = (2048, 512, 5, 2, 1)
    with Device(key) as dev:
        route = dev.plan.step_route(2, 1)
        assert dev.plan.native_fft and (route["rows_fwd"], route["Ny"], route["shift_bwd_rows"]) == ("1152", 2304, 4), route
        assert route["pooled_supported"] and route["pooled_column_io"], route
        check("native 4096x1024 R=4", dev.single(0, (1.25, -2.5), LOG_NORM), key, [((1.25, -2.5), LOG_NORM)])


def test_shift_backward_tiling_narrow():
    """W = 72: R = 1 with eight row segments of 32 threads per block, 14 of them idle."""
    key = (24, 36, 5, 2, 3)
    cals = [((1.25, -2.5), LOG_NORM)] * 3
    with Device(key) as dev:
        route = dev.plan.step_route(2, 1)
        assert dev.plan.native_fft and route["shift_bwd_rows"] == 1 and route["pooled_supported"], route
        check("narrow W=72", dev.single(0, *cals[0]), key, cals[:1])
        batch = dev.batch(cals)
        assert_same_bits(batch, dev.loop(cals))
        check("narrow W=72 batch of 3", batch, key, cals)


# ---------------------------------------------------------------------------------------------------------------------
# D. the generic route: launch_shift_fwd -> convolution -> poisson_pooled_kernel -> launch_shift_bwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["fft", "direct"])
@pytest.mark.parametrize("U,shape", [(5, (12, 20, 3)), (8, (12, 20, 3)), (2, (25, 40, 5))], ids=["u5", "u8", "u2-odd-height"])
def test_generic_route(U, shape, method):
    """Factors the fused launches do not take (5, 8) and a counts grid with an odd number of rows (H % (2 U) != 0)."""
    key = (*shape, U, 3)
    with Device(key, method=method) as dev:
        route = dev.plan.step_route(U, 3)
        assert dev.plan.method == method and not route["pooled_supported"] and route["batched"] == 0, route
        label = f"generic {method} u{U}-{'x'.join(map(str, shape))}"
        check(f"{label} uncalibrated", dev.single(0), key, [(None, None)])
        check(f"{label} calibrated", dev.single(0, (1.25, -2.5), LOG_NORM), key, [((1.25, -2.5), LOG_NORM)])
        batch = dev.batch(BATCH_CALS, fill=0.5, grad_scale=0.5)  # (the per-dataset calls inside the library)
        assert_same_bits(batch, dev.loop(BATCH_CALS, fill=0.5, grad_scale=0.5))
        check(f"{label} batch of 3 accumulate", batch, key, BATCH_CALS, fill=0.5, grad_scale=0.5)


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_two_calibrated_components(method):
    """Two flux components under one calibration on one plan: d loss / d shift is the sum over both
    (`launch_finalize_multi(..., c > 0)`), every component has its own gradient image."""
    U, shape = 2, (24, 40, 5)
    key = (*shape, U, 2)
    shift = (1.25, -2.5)
    flux, datasets = inputs(*key)
    flux2 = np.ascontiguousarray(flux[::-1, ::-1]) * np.float32(0.5)
    a, b = datasets
    r = step_oracle.step_oracle([flux, flux2], [a["exposure"], b["exposure"]], [a["psf"], b["psf"]], a["background"], a["counts"], U,
                                shift=shift, log_norm=LOG_NORM)
    assert step_oracle.clip_margin(r["pooled"]) >= 1e-3
    with Device(key, method=method) as dev:
        da, db = dev.ds
        fluxes = [dev.flux, torch.from_numpy(flux2).to(DEV)]
        grads = [dev.grad_image(NAN), dev.grad_image(NAN)]
        cal, loss = dev.calibration(shift, LOG_NORM), torch.full((1,), NAN, device=DEV)
        dev.plan.npred_poisson_fwd_bwd(fluxes, [da["exposure"], db["exposure"]], [da["khat"], db["khat"]], da["background"], da["counts"],
                                       da["stirling"], loss, grads=grads, upsampling=U, calibration=cal)
        torch.cuda.synchronize()
        errs = [rel_linf(g.cpu().numpy(), want) for g, want in zip(grads, r["grad_flux"])]
        gs, gn = cal[2].cpu().numpy().astype(np.float64), float(cal[3])
        print(f"STEP-MATRIX two components {method}: flux gradients {errs[0]:.1e} {errs[1]:.1e}, loss {abs(float(loss) / r['loss'] - 1):.1e}, "
              f"shift {np.abs(gs - r['grad_shift']).max() / np.abs(r['grad_shift']).max():.1e}, norm {abs(gn / r['grad_log_norm'] - 1):.1e}")
        assert abs(float(loss) / r["loss"] - 1) <= 5e-6
        assert max(errs) < 1e-5, errs
        np.testing.assert_allclose(gs, r["grad_shift"], rtol=1e-4, atol=2e-5 * np.abs(r["grad_shift"]).max())
        assert abs(gn / r["grad_log_norm"] - 1) <= 2e-5


@pytest.mark.parametrize("U,shape", [(2, (24, 40, 5)), (4, (24, 40, 5))], ids=["u2", "u4"])
def test_npred_out_takes_the_separate_kernels(U, shape):
    """A caller that asks for the predicted counts gets the un-fused kernels: the same numbers, and n itself."""
    key = (*shape, U, 3)
    shift = (1.25, -2.5)
    with Device(key) as dev:
        npred = torch.full(shape[:2], NAN, device=DEV)
        got = dev.single(0, shift, LOG_NORM, npred_out=npred)
        check(f"npred_out u{U}", got, key, [(shift, LOG_NORM)])
        err = rel_linf(npred.cpu().numpy(), ref(key, 0, shift, LOG_NORM)["npred"])
        assert err < 1e-5, err

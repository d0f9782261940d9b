"""The native FFT convolution (csrc/fftnative.hip) by KERNEL, not by image size: every row-transform length (25) at its edges,
every column length (15) and every entry of the column kernel table, the un-up-sampled likelihood step on every row
schedule, and unit impulses on an empty image -- against float64.  The cases come from tests/fft_length_cases.py, whose
coverage tests/test_fft_length_cases_host.py checks on the CPU; every test here first asks the library which kernels it is
about to run (`ConvPlan.fft_route`, jd_conv_plan_fft_route) and asserts that they are the ones the case means.

Bounds.  Convolution and adjoint (A, B): the rule of tests/test_gpu_fft_wide.py -- each case measures the error e_roc of the
rocFFT plan (JD_FFT_NATIVE=0) on the same inputs against float64 (scipy.signal.fftconvolve), and the native result must lie
within max(2e-6, 2 e_roc) of float64; <conv x, y> = <x, adj y> to 1e-5.  The measured figures (one FFT-LENGTHS line per case)
are in profiles/fft_lengths/README.md.  Likelihood step (C): tests/step_oracle.py at the bounds of
tests/test_gpu_walk_chain.py, 1e-5 on the gradient and npred images and 5e-6 on the loss; the batch of three bit for bit
against its per-dataset calls.  Impulses (D): 2e-6 x the largest tap, on the footprints and -- in absolute terms -- away
from them."""
import functools

import numpy as np
import pytest
import torch

import fft_length_cases as flc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGE_TOL, LOSS_TOL, IDENTITY_TOL = 1e-5, 5e-6, 1e-5
FILL = 0.5


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)  # (the cached inputs are read-only)


def _ids(cases):
    return [c["id"] for c in cases]


def _set(jd_option, case):
    for key, value in case["options"].items():
        jd_option(key, value)


def _native_plan(case):
    """The plan of a case, after the assertion that it runs the kernels the case is about."""
    from jolideco_amd.ops import ConvPlan

    plan = ConvPlan(*case["shape"], *case["kshape"], DEV, method="fft")
    assert plan.native_fft
    route = plan.fft_route(1)
    assert (route["Nx"], route["Ny"]) == (case["Nx"], case["Ny"]), route
    assert (route["col_lanes"], route["col_block"], route["col_static"]) == case["cols"], route
    # (a launch of at least three row pairs per compute unit runs short rows on the one-wave kernels: the long columns)
    rows = flc.row_schedule(case["Nx"], case["shape"][1], case["tiny"], case["Hh"], torch.cuda.get_device_properties(0).multi_processor_count)
    assert rows == case["rows"] and (route["rows_fwd"], route["rows_inv"]) == (rows, rows), route
    return plan


def _convolutions(plan, image, scale, psf, y=None):
    """conv, adjoint accumulated onto a filled image (less the fill), adjoint[, adjoint of y] -- numpy"""
    khat = plan.psf_spectrum(_dev(psf))
    x, s = _dev(image), _dev(scale)
    conv = plan.conv_same(x, s, khat)
    base = torch.full(image.shape, FILL, device=DEV)
    acc = plan.conv_same_adjoint(x, s, khat, grad_image=base, accumulate=True)
    adj = plan.conv_same_adjoint(x, s, khat)
    out = [conv, acc, adj] + ([plan.conv_same_adjoint(_dev(y), s, khat)] if y is not None else [])
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    out[1] = out[1] - FILL
    return out


@functools.lru_cache(maxsize=None)
def _baseline(shape, kshape):
    """Per geometry, once: the float64 convolution and adjoint, and the errors of the rocFFT plan against them"""
    from jolideco_amd import _hip
    from jolideco_amd.ops import ConvPlan

    image, scale, _ = flc.conv_inputs(shape)
    psf = flc.general_psf(kshape)
    ref, ref_adj = flc.conv_references(image, scale, psf)
    with _hip.options(JD_FFT_NATIVE=0):
        plan = ConvPlan(*shape, *kshape, DEV, method="fft")
        assert not plan.native_fft
        conv, acc, adj = _convolutions(plan, image, scale, psf)
        plan.close()
    e_roc = (flc.rel_linf(conv, ref), flc.rel_linf(acc, ref_adj), flc.rel_linf(adj, ref_adj))
    return ref, ref_adj, e_roc


def _check_convolution(case, jd_option):
    shape, kshape = case["shape"], case["kshape"]
    ref, ref_adj, e_roc = _baseline(shape, kshape)
    image, scale, y = flc.conv_inputs(shape)
    psf = flc.general_psf(kshape)
    _set(jd_option, case)
    plan = _native_plan(case)
    conv, acc, adj, adj_y = _convolutions(plan, image, scale, psf, y)
    plan.close()
    figures, failures = [], []
    for name, got, want, e_r in (("conv", conv, ref, e_roc[0]), ("adjoint+=", acc, ref_adj, e_roc[1]), ("adjoint", adj, ref_adj, e_roc[2])):
        ok, e_nat = flc.within_bound(got, want, e_r)
        figures.append(f"{name} native {e_nat:.2e} rocFFT {e_r:.2e}")
        if not ok:
            failures.append(f"{name}: {e_nat:.2e} > {flc.error_bound(e_r):.2e} against float64")
    # the two are transposes of each other: <conv(x), y> = <x, adjoint(y)> (the scale image on the input side of both)
    lhs, rhs = float((conv.astype(np.float64) * y).sum()), float((image.astype(np.float64) * adj_y).sum())
    identity = abs(lhs - rhs) / abs(lhs)
    print(f"FFT-LENGTHS {case['id']} (Nx {case['Nx']}, Ny {case['Ny']}, rows {case['rows']}, columns {case['cols']}): "
          + "; ".join(figures) + f"; identity {identity:.1e}")
    assert not failures, "; ".join(failures)
    assert identity <= IDENTITY_TOL, identity


# ---- A: rows -------------------------------------------------------------------------------------------------------------
ROWS, ROWS_TINY = flc.row_cases(), flc.row_cases(tiny=True)


@pytest.mark.parametrize("case", ROWS, ids=_ids(ROWS))
def test_every_row_length_at_its_edges(case, jd_option):
    """Full width (W + halo == Nx; kw = 1: no padding column at all), a ragged width, the smallest width of the length."""
    _check_convolution(case, jd_option)


@pytest.mark.parametrize("case", ROWS_TINY, ids=_ids(ROWS_TINY))
def test_every_row_length_up_to_1024_on_the_one_wave_kernels(case, jd_option):
    assert case["rows"] == "tiny"
    _check_convolution(case, jd_option)


# ---- B: columns ----------------------------------------------------------------------------------------------------------
COLS = flc.column_cases()


@pytest.mark.parametrize("case", COLS, ids=_ids(COLS))
def test_every_column_length_and_table_entry(case, jd_option):
    """Exact fit (Hh + kh - 1 == Ny), its odd-H neighbour, the smallest H; Hh == kh; Ny == 2 kh; the columns per block forced
    on the lengths with compile-time entries (among them the generic kernels on those lengths); Nx = Ny = 1152."""
    _check_convolution(case, jd_option)


def test_a_forced_block_beyond_the_launch_bounds_of_its_kernel_is_not_taken(jd_option):
    """Ny = 2048 with JD_FFT_NATIVE = 8 has no compile-time entry and would be 128 x 8 = 1024 threads: the default stands.  (The
    convolution on that route is the cols-forced case of this geometry above.)"""
    case = next(c for c in COLS if c["kind"] == "cols-forced" and c["Ny"] == 2048 and c["options"]["JD_FFT_NATIVE"] == 8)
    _set(jd_option, case)
    plan = _native_plan(case)
    route = plan.fft_route(1)
    plan.close()
    assert (route["col_lanes"], route["col_block"], route["col_static"]) == (128, 4, 1), route


def test_the_route_query_refuses_other_plans(jd_option):
    from jolideco_amd.ops import ConvPlan

    jd_option("JD_FFT_NATIVE", 0)
    for method in ("fft", "direct"):
        plan = ConvPlan(48, 64, 9, 9, DEV, method=method)
        with pytest.raises(RuntimeError, match="libjolideco_hip error -1"):
            plan.fft_route(1)
        plan.close()


# ---- C: the un-up-sampled likelihood step --------------------------------------------------------------------------------
STEPS = flc.step_cases()
N_BATCH = 3


@functools.lru_cache(maxsize=None)
def _step_inputs(shape):
    """flux and, per dataset, (exposure, background, counts, stirling, psf): positive, as in tests/test_gpu_walk_chain.py"""
    from jolideco_amd.ops import stirling_mean

    H, W = shape
    rs = np.random.RandomState(5 + 1000 * H + W)
    flux = rs.gamma(5.0, size=shape).astype(np.float32)
    data = []
    for i in range(N_BATCH):
        exposure = ((1.0 + 0.1 * i) * (1.0 + 0.4 * np.linspace(-1, 1, H)[:, None] * np.ones(shape))).astype(np.float32)
        counts = rs.poisson(5.0, size=shape).astype(np.float32)
        data.append((exposure, np.full(shape, 0.5 + 0.1 * i, dtype=np.float32), counts, stirling_mean(counts),
                     flc.general_psf(flc.STEP_K, seed=7 + i)))
    return flux, tuple(data)


@functools.lru_cache(maxsize=None)
def _step_oracle(shape):
    from step_oracle import step_oracle

    flux, data = _step_inputs(shape)
    return [step_oracle(flux, d[0], d[4], d[1], d[2], 1) for d in data]


@pytest.mark.parametrize("case", STEPS, ids=_ids(STEPS))
def test_likelihood_step_on_every_row_schedule(case, jd_option):
    """`fftn_poisson_step` (jd_npred_poisson_fwd_bwd, one dataset: written, and accumulated onto a filled image) and
    `fftn_poisson_step_batch` (ConvPlan.npred_poisson_batch_fwd_bwd, three datasets: bit for bit against the per-dataset calls
    with `accumulate` from the second on, and against the oracle), upsampling = 1."""
    shape = case["shape"]
    flux_h, data_h = _step_inputs(shape)
    oracle = _step_oracle(shape)
    _set(jd_option, case)
    plan = _native_plan(case)
    assert plan.fft_route(N_BATCH)["rows_fwd"] == case["rows"]
    flux = _dev(flux_h)
    data = [tuple(_dev(a) for a in d[:3]) + (d[3], plan.psf_spectrum(_dev(d[4]))) for d in data_h]

    def single(d, grad, accumulate, grad_scale=1.0, npred=None):
        exposure, background, counts, stirling, khat = data[d]
        loss = torch.zeros(1, device=DEV)
        plan.npred_poisson_fwd_bwd([flux], [exposure], [khat], background, counts, stirling, loss, grads=[grad],
                                   accumulate=accumulate, grad_scale=grad_scale, npred_out=npred)
        return loss

    def loop(fill, accumulate):
        grad = torch.full(shape, fill, device=DEV)
        losses = [single(d, grad, accumulate or d > 0) for d in range(N_BATCH)]
        return grad, torch.cat(losses)

    def batch(fill, accumulate):
        grad = torch.full(shape, fill, device=DEV)
        losses = [torch.zeros(1, device=DEV) for _ in range(N_BATCH)]
        plan.npred_poisson_batch_fwd_bwd(flux, [d[0] for d in data], [d[4] for d in data], [d[1] for d in data], [d[2] for d in data],
                                         [d[3] for d in data], losses, grad=grad, accumulate=accumulate)
        return grad, torch.cat(losses)

    figures, failures = [], []

    def compare(name, got, want, tol, relative_scalar=False):
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        e = float(np.max(np.abs(got / want - 1))) if relative_scalar else flc.rel_linf(got, want)
        figures.append(f"{name} {e:.2e}")
        if not e < tol:
            failures.append(f"{name}: {e:.2e} >= {tol:.0e}")

    # one dataset: the fused step, written over a filled image and accumulated onto it with a scale
    g0, l0 = oracle[0]["grad_flux"], oracle[0]["loss"]
    grad = torch.full(shape, FILL, device=DEV)
    loss = single(0, grad, False)
    compare("gradient", grad, g0, IMAGE_TOL)
    compare("loss", loss, np.array([l0]), LOSS_TOL, True)
    grad = torch.full(shape, FILL, device=DEV)
    loss = single(0, grad, True, grad_scale=0.5)
    compare("gradient+=", grad, FILL + 0.5 * g0, IMAGE_TOL)
    compare("loss+=", loss, np.array([l0]), LOSS_TOL, True)
    # (with an npred image the step runs unfused: convolution, Poisson pass, adjoint)
    grad, npred = torch.full(shape, FILL, device=DEV), torch.empty(shape, device=DEV)
    loss = single(0, grad, False, npred=npred)
    compare("npred", npred, oracle[0]["npred"], IMAGE_TOL)
    compare("gradient (unfused)", grad, g0, IMAGE_TOL)
    compare("loss (unfused)", loss, np.array([l0]), LOSS_TOL, True)
    # a batch of three
    g_sum, l_all = sum(o["grad_flux"] for o in oracle), np.array([o["loss"] for o in oracle])
    for fill, accumulate, tag in ((-7.0, False, "batch"), (FILL, True, "batch+=")):
        grad_b, losses_b = batch(fill, accumulate)
        grad_l, losses_l = loop(fill, accumulate)
        torch.cuda.synchronize()
        assert torch.equal(grad_b, grad_l) and torch.equal(losses_b, losses_l), f"{tag}: not the bits of the per-dataset calls"
        compare(f"{tag} gradient", grad_b, g_sum + (fill if accumulate else 0.0), IMAGE_TOL)
        compare(f"{tag} losses", losses_b, l_all, LOSS_TOL, True)
    plan.close()
    print(f"FFT-LENGTHS {case['id']} (Nx {case['Nx']}, Ny {case['Ny']}, rows {case['rows']}): " + "; ".join(figures))
    assert not failures, "; ".join(failures)


# ---- D: impulses on an empty image ---------------------------------------------------------------------------------------
def test_impulses_on_an_empty_image(jd_option):
    """Unit impulses at the four corners, in rows Hh - 1 and Hh (the seam between the two image rows packed into one complex
    transform) and in the last column, PSF 9 x 13 with taps 1 + index: a dropped or mirrored tap, or leakage across the seam,
    that a random image of large dynamic range could hide under its own maximum."""
    psf = flc.impulse_psf()
    failures = []
    for case in flc.impulse_cases():
        H, W = case["shape"]
        plan = _native_plan(case)
        khat = plan.psf_spectrum(_dev(psf))
        x = _dev(flc.impulse_image(H, W))
        conv, adj = plan.conv_same(x, None, khat), plan.conv_same_adjoint(x, None, khat)
        torch.cuda.synchronize()
        plan.close()
        for name, got, adjoint in (("conv", conv, False), ("adjoint", adj, True)):
            ref, inside = flc.impulse_reference(H, W, psf, adjoint)
            bad, e_in, e_out = flc.impulse_failures(got.cpu().numpy(), ref, inside, float(psf.max()))
            print(f"FFT-LENGTHS {case['id']} {name}: footprints {e_in:.2e}, outside {e_out:.2e} (bound {2e-6 * psf.max():.2e})")
            failures += [f"{case['id']} {name} {b}" for b in bad]
    assert not failures, "; ".join(failures)

"""The native FFT convolution (csrc/fftnative.hip) beyond 4608-point rows and 2304-point columns: row transforms up to 9216
points on the 768-thread "generic-huge" kernels (6144 = 16 16 8 3, 8192 = 16 8 8 8, 9216 = 16 8 8 9), column transforms of
4096 = 16 16 16 and 4608 = 8 8 8 9 points on four waves per column -- images up to 9216 columns x 2 * 4608 rows less the PSF's
halo, which ran on rocFFT plans before.

1. convolution and adjoint against float64 and against the rocFFT plan of the same build (JD_FFT_NATIVE=0);
2. the up-sampled, calibrated likelihood step (the harness of tests/test_gpu_upsampled_step.py) on flux grids of those widths;
3. a joint fit of three 5000-column observations against the oracle.

Bounds of 1.: the library's 2e-6 (relative L-inf against float64) was set on transforms up to 4608 x 2304 points.  Each case
measures the error e_roc of the rocFFT plan on the same inputs; the native result must lie within max(2e-6, 2 e_roc) of
float64 (the 2: a different, equally rounded order of operations) and within that bound plus e_roc of rocFFT's result.  The
measured errors are in profiles/fft_wide/README.md.

An image half must hold the PSF (`fftn_supported`: Hh >= kh, at every width), so the 33 x 17 PSF runs on 66 rows and the
17 x 17 PSF on 34."""
import numpy as np
import pytest
import torch

from conftest import rel_linf
from test_gpu_upsampled_step import BATCH_CALS, Device, assert_same_bits, check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHIFT, LOG_NORM = (0.2, -0.15), float(np.log(1.1))

# (image shape, PSF shape, Nx, Ny, the rows run "generic-huge")
CASES = [((24, 4800), (5, 5), 6144, 32, True), ((66, 6100), (33, 17), 6144, 72, True), ((26, 8000), (9, 9), 8192, 32, True),
         ((34, 8192), (17, 17), 9216, 64, True), ((25, 9203), (5, 7), 9216, 32, True),  # odd rows, ragged width
         # columns of 4096 and 4608 points: four waves per column
         ((4700, 64), (9, 9), 72, 4096, False), ((8192, 64), (17, 17), 72, 4608, False), ((8001, 68), (9, 5), 72, 4096, False),
         ((9000, 64), (9, 9), 72, 4608, False),
         ((4700, 4800), (9, 9), 6144, 4096, True)]  # both


def _psf(kshape, seed):
    rs = np.random.RandomState(seed)
    psf = rs.uniform(0.0, 1.0, size=kshape) ** 3  # a general (full-rank) kernel
    return (psf / psf.sum()).astype(np.float32)


@pytest.mark.parametrize("shape,kshape,Nx,Ny,huge", CASES, ids=[f"{c[0][0]}x{c[0][1]}_k{c[1][0]}x{c[1][1]}" for c in CASES])
def test_wide_convolution_and_adjoint_match_float64_and_rocfft(jd_option, shape, kshape, Nx, Ny, huge):
    from scipy.signal import fftconvolve

    from jolideco_amd.ops import ConvPlan

    H, W = shape
    rs = np.random.RandomState(H + W)
    image = rs.gamma(2.0, size=shape).astype(np.float32)
    image[rs.randint(0, H, 20), rs.randint(0, W, 20)] += 500.0  # point sources: a large dynamic range
    scale = rs.uniform(0.5, 1.5, size=shape).astype(np.float32)
    psf = _psf(kshape, 7)
    oy, ox = (kshape[0] - 1) // 2, (kshape[1] - 1) // 2
    full = fftconvolve(image.astype(np.float64) * scale, psf.astype(np.float64), mode="full")
    ref = full[oy:oy + H, ox:ox + W]
    full_adj = fftconvolve(image.astype(np.float64), psf[::-1, ::-1].astype(np.float64), mode="full")
    ay, ax = kshape[0] - 1 - oy, kshape[1] - 1 - ox
    ref_adj = full_adj[ay:ay + H, ax:ax + W] * scale
    out = {}
    for native in (1, 0):
        jd_option("JD_FFT_NATIVE", native)
        plan = ConvPlan(H, W, kshape[0], kshape[1], DEV, method="fft")
        assert plan.native_fft == bool(native)
        if native:
            route = plan.step_route(1, 1)
            assert (route["Nx"], route["Ny"]) == (Nx, Ny), route
            assert not huge or route["rows_fwd"] == "generic-huge", route
        khat = plan.psf_spectrum(torch.from_numpy(psf).to(DEV))
        x, s = torch.from_numpy(image).to(DEV), torch.from_numpy(scale).to(DEV)
        conv = plan.conv_same(x, s, khat)
        base = torch.full(shape, 0.5, device=DEV)
        adj = plan.conv_same_adjoint(x, s, khat, grad_image=base.clone(), accumulate=True)
        adj0 = plan.conv_same_adjoint(x, s, khat)
        torch.cuda.synchronize()
        out[native] = (conv.cpu().numpy(), adj.cpu().numpy() - 0.5, adj0.cpu().numpy())
        plan.close()
    figures, failures = [], []
    for i, (name, want) in enumerate((("conv", ref), ("adjoint (accumulated)", ref_adj), ("adjoint", ref_adj))):
        e_nat, e_roc = rel_linf(out[1][i], want), rel_linf(out[0][i], want)
        bound = max(2e-6, 2.0 * e_roc)
        between = rel_linf(out[1][i], out[0][i])
        figures.append(f"{name}: native {e_nat:.2e}, rocFFT {e_roc:.2e}, native against rocFFT {between:.2e}")
        if not e_nat <= bound:
            failures.append(f"{name}: {e_nat:.2e} > {bound:.2e} against float64")
        if not between <= bound + e_roc:
            failures.append(f"{name}: {between:.2e} > {bound + e_roc:.2e} against rocFFT")
    print(f"FFT-WIDE {H}x{W} k{kshape[0]}x{kshape[1]} (Nx {Nx}, Ny {Ny}): " + "; ".join(figures))
    assert not failures, "; ".join(failures)
    # the two are transposes of each other: <conv(x), y> = <x, adjoint(y)>
    y = rs.uniform(size=shape).astype(np.float32)
    jd_option("JD_FFT_NATIVE", 1)
    plan = ConvPlan(H, W, kshape[0], kshape[1], DEV, method="fft")
    assert plan.native_fft
    khat = plan.psf_spectrum(torch.from_numpy(psf).to(DEV))
    adj_y = plan.conv_same_adjoint(torch.from_numpy(y).to(DEV), torch.from_numpy(scale).to(DEV), khat).cpu().numpy()
    plan.close()
    lhs = float((out[1][0].astype(np.float64) * y).sum())
    rhs = float((image.astype(np.float64) * adj_y).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)


# (U, (counts rows, counts columns, PSF size in counts pixels)): flux rows of 5200 (6144 points), 8192 (9216), 5400 (6144),
# 8192 (9216) and 5202 pixels (ragged), and a 4800 x 64 flux grid (Ny = 4096) with pooled column I/O
STEPS = [(2, (24, 2600, 5)), (2, (24, 4096, 5)), (3, (24, 1800, 5)), (4, (24, 2048, 5)), (2, (24, 2601, 5)), (2, (2400, 32, 5))]


@pytest.mark.parametrize("U,shape", STEPS, ids=[f"u{U}-{'x'.join(map(str, s))}" for U, s in STEPS])
def test_wide_likelihood_step(U, shape, jd_option):
    """The sequence of test_factor_schedule_pooled_io: one dataset uncalibrated, calibrated, both accumulating onto a filled
    gradient; a batch of three bit for bit against its per-dataset calls and against the oracle; the batch again with
    JD_FFT_BATCH=0."""
    Hd, Wd, k = shape
    key = (Hd, Wd, k, U, 3)
    label = f"wide u{U}-{'x'.join(map(str, shape))}"
    columns = Hd > 1000

    def assert_route(route):
        assert route["pooled_supported"], route
        if columns:
            assert route["Ny"] == 4096 and route["pooled_column_io"], route
        else:
            assert (route["rows_fwd"], route["rows_pooled"]) == ("generic-huge", "generic-huge"), route

    with Device(key) as dev:
        assert dev.plan.native_fft
        route = dev.plan.step_route(U, 1)
        assert_route(route)
        assert (route["shift_bwd_rows"] > 0) == ((U * Wd) % 4 == 0), route  # (ragged rows: the scalar shift kernels)
        check(f"{label} uncalibrated", dev.single(0), key, [(None, None)])
        check(f"{label} calibrated", dev.single(0, SHIFT, LOG_NORM), key, [(SHIFT, LOG_NORM)])
        check(f"{label} calibrated accumulate", dev.single(0, SHIFT, LOG_NORM, grad=dev.grad_image(0.5), accumulate=True, grad_scale=0.5),
              key, [(SHIFT, LOG_NORM)], fill=0.5, grad_scale=0.5)
        check(f"{label} uncalibrated accumulate", dev.single(0, grad=dev.grad_image(0.5), accumulate=True, grad_scale=0.5),
              key, [(None, None)], fill=0.5, grad_scale=0.5)
        route = dev.plan.step_route(U, 3)
        assert_route(route)
        assert route["batched"] == 1, route
        batch = dev.batch(BATCH_CALS)
        assert_same_bits(batch, dev.loop(BATCH_CALS))
        check(f"{label} batch of 3", batch, key, BATCH_CALS)
        batch = dev.batch(BATCH_CALS, fill=0.5, grad_scale=0.5)
        assert_same_bits(batch, dev.loop(BATCH_CALS, fill=0.5, grad_scale=0.5))
        check(f"{label} batch of 3 accumulate", batch, key, BATCH_CALS, fill=0.5, grad_scale=0.5)
        jd_option("JD_FFT_BATCH", 0)
        assert dev.plan.step_route(U, 3)["batched"] == 0
        assert_same_bits(dev.batch(BATCH_CALS), dev.loop(BATCH_CALS))


def test_wide_joint_fit_matches_the_oracle(monkeypatch):
    """Three epochs of a joint fit of three 16 x 5000 observations (Gaussian PSFs of 5 x 5, 7 x 7 and 7 x 7 pixels: an image
    half of 8 rows holds them) through the native FFT path: one plan, 6144-point rows, the batched joint step -- whose last
    launch, `fftn_rows_inv_batch_kernel`, sums the datasets' gradients in the output rows on this schedule."""
    from jolideco_amd import MAPDeconvolver, SpatialFluxComponent, UniformPrior
    from jolideco_amd.data import gaussian_kernel, synthetic_observations
    from oracle import cpu_ref

    monkeypatch.setenv("JOLIDECO_CONV_METHOD", "fft")
    datasets, _, flux_init = synthetic_observations(shape=(16, 5000), n_obs=3, seed=2)
    for ds, (sigma, size) in zip(datasets.values(), ((1.0, 5), (1.25, 7), (1.5, 7))):
        ds["psf"] = gaussian_kernel(sigma, (size, size)).astype(np.float32)
    comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=UniformPrior())
    deco = MAPDeconvolver(n_epochs=3, display_progress=False, device=DEV, fit_mode="joint")
    session = deco.session(datasets, components=comp)
    plans = {m.plan for models in session.total_loss.poisson_loss.npred_models_all for m in models.values()}
    assert all(p.native_fft for p in plans) and session.batch_joint
    assert all(p.step_route(1, 3)["rows_fwd"] == "generic-huge" for p in plans)
    res = deco.run(datasets, components=comp)
    final, _ = cpu_ref.map_fit_joint(datasets, {"flux": flux_init}, {"flux": cpu_ref.UniformPriorRef()}, n_epochs=3)
    assert rel_linf(res.flux_total, final["flux"]) < 1e-5

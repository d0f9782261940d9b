"""GPU: flux components with DIFFERENT up-sampling factors in one fit (jd_npred_poisson_mixed_fwd_bwd).

The reference builds one NPredModel per component with that component's `upsampling_factor`
(jolideco/models/npred.py:279-295), sum-pools each convolution to the counts grid before the clip (:181-191) and adds
the clipped terms (:241-261).  Here every component runs on its own convolution plan and ONE Poisson launch over the
counts grid reads every plan's buffer with that plan's geometry.  Yardsticks: the live-reference fixture
tests/golden/mixed_upsampling.npz (tools/make_golden_mixed_upsampling.py) and oracle/cpu_ref.py, which reproduces the
reference bit for bit on such fits (tests/test_mixed_upsampling_golden.py).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_linf, unpack_datasets
from mixed_upsampling_cases import clip_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (40, 44)


def _gmm(means, covs, weights):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    return GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))


def _trace_close(trace, arrays, prefix="trace/", rtol=2e-5):  # (the tolerances of tests/test_gpu_fit.py)
    for key, ref in arrays.items():
        if key.startswith(prefix):
            name = key[len(prefix):]
            np.testing.assert_allclose(trace[name], ref, rtol=rtol, atol=1e-6, err_msg=name)


def _components(m, u_ext, u_pts, generator=None):
    from jolideco_amd import FluxComponents, GMMPatchPrior, InverseGammaPrior, SpatialFluxComponent

    kwargs = {} if generator is None else {"generator": generator}
    comps = FluxComponents()
    comps["extended"] = SpatialFluxComponent.from_numpy(
        flux=m["init/extended"], upsampling_factor=u_ext,
        prior=GMMPatchPrior(gmm=_gmm(m["gmm/means"], m["gmm/covariances"], m["gmm/weights"]), **kwargs),
    )
    comps["points"] = SpatialFluxComponent.from_numpy(flux=m["init/points"], upsampling_factor=u_pts,
                                                      prior=InverseGammaPrior(alpha=10, beta=1.5))
    return comps


# ---------------------------------------------------------------------------------------------------------------------
# 1. fits against the live-reference fixture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u_ext,u_pts", [(1, 2), (3, 2)])
def test_fit_matches_the_live_reference(golden, conv_method, u_ext, u_pts):
    """MAPDeconvolver.run, sequential, 4 epochs, against the reference's fit: up-sampled flux of each component at
    rel L-inf < 1e-5, the trace at the tolerances of tests/test_gpu_fit.py, flux_total on the counts grid."""
    from jolideco_amd import MAPDeconvolver

    m = golden("mixed_upsampling")
    tag = f"u{u_ext}{u_pts}"
    res = MAPDeconvolver(n_epochs=4, display_progress=False, device=DEV).run(
        unpack_datasets(m), components=_components(m, u_ext, u_pts)
    )
    for name in ("extended", "points"):
        err = rel_linf(res.components[name].flux_upsampled_numpy, m[f"{tag}/final_upsampled/{name}"])
        print(f"mixed up-sampling {tag} / {conv_method} / {name}: rel L-inf {err:.2e}")
        assert err < 1e-5, (name, err)
    _trace_close(res.trace_loss, m, prefix=f"{tag}/trace/")
    assert res.flux_total.shape == SHAPE
    assert rel_linf(res.flux_total, m[f"{tag}/flux_total"]) < 1e-5


@pytest.mark.parametrize("native_fft", [1, 0])
def test_one_step_matches_the_live_reference(golden, monkeypatch, jd_option, native_fft):
    """npred, loss and d loss / d flux_c of one step, factors (1, 2), against NPredModels.evaluate + PoissonNLLLoss autograd
    of the reference; on the FFT method with the native transforms and with rocFFT, whose padded grid gives every plan
    its own row pitch and crop offset."""
    from jolideco_amd import NPredModels
    from jolideco_amd.ops import ConvPlan, stirling_mean

    monkeypatch.setenv("JOLIDECO_CONV_METHOD", "fft")
    jd_option("JD_FFT_NATIVE", native_fft)
    monkeypatch.setattr(ConvPlan, "_cache", {})  # (the option is read when a plan is created: no plan of another test)
    m = golden("mixed_upsampling")
    data = unpack_datasets(m)["o0"]
    models = NPredModels.from_dataset_numpy(dataset=data, components=_components(m, 1, 2), device=DEV)
    plans = [model.plan for model in models.values()]
    assert plans[0] is not plans[1] and all(p.method == "fft" for p in plans)
    if not native_fft:
        assert all((p.Hp, p.Wp) != (p.H, p.W) for p in plans)
    names = ("extended", "points")
    fluxes = [torch.from_numpy(m[f"step/flux/{n}"]).to(DEV) for n in names]
    grads = [torch.full_like(f, 7.0) for f in fluxes]  # (overwritten: accumulate=False)
    counts = torch.from_numpy(data["counts"]).to(DEV)
    loss, npred = torch.zeros(1, device=DEV), torch.empty(SHAPE, device=DEV)
    models.fwd_bwd(fluxes, counts, stirling_mean(data["counts"]), loss, grads=grads, npred_out=npred)
    np.testing.assert_allclose(float(loss), float(m["step/loss"]), rtol=3e-6)
    assert rel_linf(npred.cpu().numpy(), m["step/npred"]) < 1e-5
    for n, g in zip(names, grads):
        assert rel_linf(g.cpu().numpy(), m[f"step/grad_flux/{n}"]) < 1e-5, n
    torch.cuda.synchronize()
    for plan in plans:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. one step at a size that fills the device
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_step(datasets, fluxes_np, ups, dtype):
    """Summed loss per dataset and d (sum of losses) / d flux_c by oracle/cpu_ref.py autograd in `dtype`."""
    from oracle import cpu_ref

    with cpu_ref.precision(dtype):
        fluxes = tuple(cpu_ref._tensor(f[None, None]).requires_grad_(True) for f in fluxes_np)
        losses = []
        for data in datasets.values():
            d = cpu_ref.DatasetRef.from_numpy(data, ["extended", "points"], list(ups))
            loss = d.loss(fluxes)
            loss.backward()
            losses.append(float(loss.detach()))
        return losses, [f.grad.numpy()[0, 0].astype(np.float64) for f in fluxes]


def _big_case(n_obs=2, shape=(1024, 1024)):
    from jolideco_amd.data import instrument_like_psf, synthetic_observations

    datasets, truth, flux_init = synthetic_observations(shape=shape, n_obs=n_obs, seed=0)
    for i, d in enumerate(datasets.values()):
        d["psf"] = {"extended": d["psf"], "points": instrument_like_psf(i, (9, 9))}
    rs = np.random.RandomState(5)
    init_pts = rs.gamma(2, size=shape) * 0.2
    return datasets, flux_init, init_pts


def test_one_step_at_1024_matches_the_oracle():
    """1024^2 counts, 2 datasets, factors (1, 2): "extended" with a rank-1 17-tap Gaussian PSF on the 1024^2 grid,
    "points" with a general 9x9 PSF (18x18 after its up-sampling) on the 2048^2 grid; the second dataset accumulates.
    Losses at rtol 3e-6 and both gradients at rel L-inf < 1e-5 against the float32 oracle, the tolerance form of
    tests/test_gpu_baseline_parity.py; no arbitration by float64 is needed at this size.

    Measured on an MI355X; the two lines this test printed there (the list names the plan methods of the two components):

        1024^2 mixed (1, 2) / extended (['separable', 'fft']): gradient rel L-inf HIP-fp32 oracle 6.83e-07, HIP-float64 3.64e-07, fp32 oracle-float64 6.50e-07
        1024^2 mixed (1, 2) / points (['separable', 'fft']): gradient rel L-inf HIP-fp32 oracle 1.42e-06, HIP-float64 6.51e-07, fp32 oracle-float64 1.38e-06

    Both components are about half as far from the float64 oracle as the float32 oracle is.  The float64 distances are
    printed for the record and take no part in the assertion."""
    from jolideco_amd import FluxComponents, NPredModels, SpatialFluxComponent
    from jolideco_amd.ops import stirling_mean

    datasets, init_ext, init_pts = _big_case()
    ups = (1, 2)
    comps = FluxComponents()
    comps["extended"] = SpatialFluxComponent.from_numpy(flux=init_ext, upsampling_factor=1)
    comps["points"] = SpatialFluxComponent.from_numpy(flux=init_pts, upsampling_factor=2)
    fluxes = [c.flux_upsampled.detach().reshape(c.flux_upsampled.shape[-2:]).contiguous().to(DEV) for c in comps.values()]
    fluxes_np = [f.cpu().numpy() for f in fluxes]
    grads = [torch.zeros_like(f) for f in fluxes]
    losses = torch.zeros(len(datasets), device=DEV)
    methods = None
    for i, data in enumerate(datasets.values()):
        models = NPredModels.from_dataset_numpy(dataset=data, components=comps, device=DEV)
        methods = [m.plan.method for m in models.values()]
        counts = torch.from_numpy(data["counts"]).to(DEV)
        models.fwd_bwd(fluxes, counts, stirling_mean(data["counts"]), losses[i : i + 1], grads=grads, accumulate=i > 0)
    torch.cuda.synchronize()
    assert methods[0] == "separable" and methods[1] in ("fft", "direct")
    losses_32, grads_32 = _oracle_step(datasets, fluxes_np, ups, np.float32)
    losses_64, grads_64 = _oracle_step(datasets, fluxes_np, ups, np.float64)
    np.testing.assert_allclose(losses.cpu().numpy(), losses_32, rtol=3e-6)
    for name, g, g32, g64 in zip(("extended", "points"), grads, grads_32, grads_64):
        got = g.cpu().numpy()
        d_gpu_32, d_gpu_64, d_o_64 = rel_linf(got, g32), rel_linf(got, g64), rel_linf(g32, g64)
        print(f"1024^2 mixed (1, 2) / {name} ({methods}): gradient rel L-inf HIP-fp32 oracle {d_gpu_32:.2e}, "
              f"HIP-float64 {d_gpu_64:.2e}, fp32 oracle-float64 {d_o_64:.2e}")
        assert d_gpu_32 < 1e-5, name


# ---------------------------------------------------------------------------------------------------------------------
# 3. clip mask
# ---------------------------------------------------------------------------------------------------------------------
def test_gradient_is_masked_where_a_component_is_clipped(conv_method):
    """A component whose pooled convolution is negative on part of the counts grid: npred, the loss and both gradients
    match the oracle (whose clip passes no gradient), and the gradient WITHOUT the mask (a straight-through clip) is far
    from both -- so the agreement shows that nothing flows through the clipped pixels."""
    import torch.nn.functional as F

    from jolideco_amd import FluxComponents, NPredModels, SpatialFluxComponent
    from jolideco_amd.ops import stirling_mean
    from oracle import cpu_ref

    data, fluxes_np, ups = clip_case()
    comps = FluxComponents()
    comps["extended"] = SpatialFluxComponent.from_numpy(flux=np.ones(data["counts"].shape), upsampling_factor=ups[0])
    comps["points"] = SpatialFluxComponent.from_numpy(flux=np.ones(data["counts"].shape), upsampling_factor=ups[1])
    models = NPredModels.from_dataset_numpy(dataset=data, components=comps, device=DEV)
    fluxes = [torch.from_numpy(f).to(DEV) for f in fluxes_np]
    grads = [torch.zeros_like(f) for f in fluxes]
    loss, npred = torch.zeros(1, device=DEV), torch.empty(data["counts"].shape, device=DEV)
    counts = torch.from_numpy(data["counts"]).to(DEV)
    models.fwd_bwd(fluxes, counts, stirling_mean(data["counts"]), loss, grads=grads, npred_out=npred)

    d = cpu_ref.DatasetRef.from_numpy(data, ["extended", "points"], list(ups))

    def oracle(straight_through):
        fl = tuple(torch.from_numpy(f[None, None]).requires_grad_(True) for f in fluxes_np)
        total = d.background
        clipped = None
        for f, e, p, u in zip(fl, d.exposures, d.psfs, ups):
            pooled = F.avg_pool2d(cpu_ref.convolve_fft(f * e, p), kernel_size=u, divisor_override=1)
            term = torch.clip(pooled, 0, torch.inf)
            if straight_through:
                term = pooled + (term - pooled).detach()
            total = total + term
            clipped = (pooled < 0).numpy()[0, 0]
        value = cpu_ref.poisson_nll(total, d.counts)
        value.backward()
        return float(value.detach()), total.detach().numpy()[0, 0], [f.grad.numpy()[0, 0] for f in fl], clipped

    loss_o, npred_o, grads_o, clipped = oracle(False)
    _, _, grads_st, _ = oracle(True)
    assert 0.01 < clipped.mean() < 0.5
    np.testing.assert_allclose(float(loss), loss_o, rtol=3e-6)
    assert rel_linf(npred.cpu().numpy(), npred_o) < 1e-5
    for name, g, g_o in zip(("extended", "points"), grads, grads_o):
        assert rel_linf(g.cpu().numpy(), g_o) < 1e-5, name
    assert rel_linf(grads_st[1], grads_o[1]) > 1e-2  # (the mask matters on this input)
    assert rel_linf(grads[1].cpu().numpy(), grads_st[1]) > 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# 3b. more than two components, components that share a plan, widths the vector loads do not fit
# ---------------------------------------------------------------------------------------------------------------------
def _step_against_oracle(data, names, ups, fluxes_np):
    """One step of `data` with components `names` / factors `ups` at `fluxes_np`: HIP (loss, npred, gradients, plans)
    against oracle/cpu_ref.py autograd at the tolerances of tests/test_gpu_baseline_parity.py."""
    from jolideco_amd import FluxComponents, NPredModels, SpatialFluxComponent
    from jolideco_amd.ops import stirling_mean
    from oracle import cpu_ref

    shape = data["counts"].shape
    comps = FluxComponents()
    for name, u in zip(names, ups):
        comps[name] = SpatialFluxComponent.from_numpy(flux=np.ones(shape), upsampling_factor=u)
    models = NPredModels.from_dataset_numpy(dataset=data, components=comps, device=DEV)
    fluxes = [torch.from_numpy(f).to(DEV) for f in fluxes_np]
    grads = [torch.zeros_like(f) for f in fluxes]
    loss, npred = torch.zeros(1, device=DEV), torch.empty(shape, device=DEV)
    counts = torch.from_numpy(data["counts"]).to(DEV)
    models.fwd_bwd(fluxes, counts, stirling_mean(data["counts"]), loss, grads=grads, npred_out=npred)
    d = cpu_ref.DatasetRef.from_numpy(data, list(names), list(ups))
    fl = tuple(torch.from_numpy(f[None, None]).requires_grad_(True) for f in fluxes_np)
    npred_o = d.npred(fl)
    loss_o = cpu_ref.poisson_nll(npred_o, d.counts)
    loss_o.backward()
    np.testing.assert_allclose(float(loss), float(loss_o.detach()), rtol=3e-6)
    assert rel_linf(npred.cpu().numpy(), npred_o.detach().numpy()[0, 0]) < 1e-5
    for name, g, f in zip(names, grads, fl):
        assert rel_linf(g.cpu().numpy(), f.grad.numpy()[0, 0]) < 1e-5, name
    return [m.plan for m in models.values()]


def _small_data(shape, psfs, seed):
    rs = np.random.RandomState(seed)
    exposure = (1 + 0.3 * np.linspace(-1, 1, shape[0])).reshape(-1, 1) * (1 + 0.1 * np.linspace(-1, 1, shape[1]))
    return {"counts": rs.poisson(4.0, size=shape).astype(np.float32), "psf": psfs,
            "exposure": exposure.astype(np.float32), "background": np.full(shape, 0.5, np.float32)}, rs


@pytest.mark.parametrize("ups", [(1, 2, 2), (2, 5, 1, 2)])
def test_several_components_and_a_shared_plan(conv_method, ups):
    """Three components with factors (1, 2, 2) whose two up-sampled components have PSFs of ONE shape -- they share a plan
    object and take successive buffer slots of it --, and four components with a factor beyond 4: the generic kernel."""
    from jolideco_amd.data import gaussian_kernel, instrument_like_psf

    shape = (36, 40)
    names = [f"c{i}" for i in range(len(ups))]
    psfs = {n: (instrument_like_psf(i, (5, 5)) if i % 2 else gaussian_kernel(1.0 + 0.2 * i, (5, 5)).astype(np.float32))
            for i, n in enumerate(names)}
    data, rs = _small_data(shape, psfs, 31)
    fluxes = [(rs.gamma(3, size=(shape[0] * u, shape[1] * u)) / (u * u)).astype(np.float32) for u in ups]
    plans = _step_against_oracle(data, names, ups, fluxes)
    if conv_method != "auto":  # ("auto" gives the Gaussian and the general PSF different methods)
        twos = [p for p, u in zip(plans, ups) if u == 2]
        assert twos[0] is twos[1]


@pytest.mark.parametrize("shape", [(30, 37), (31, 42)])
def test_counts_grids_the_vector_loads_do_not_fit(conv_method, shape):
    """An odd counts width (one counts pixel per thread, scalar row pieces) and an odd height, factors (3, 2) and (1, 2)."""
    from jolideco_amd.data import gaussian_kernel, instrument_like_psf

    psfs = {"extended": gaussian_kernel(1.2, (7, 7)).astype(np.float32), "points": instrument_like_psf(1, (5, 5))}
    data, rs = _small_data(shape, psfs, 37)
    for ups in ((3, 2), (1, 2)):
        fluxes = [(rs.gamma(3, size=(shape[0] * u, shape[1] * u)) / (u * u)).astype(np.float32) for u in ups]
        _step_against_oracle(data, ("extended", "points"), ups, fluxes)


# ---------------------------------------------------------------------------------------------------------------------
# 4. accumulation and modes
# ---------------------------------------------------------------------------------------------------------------------
def _three_datasets(m):
    """Three datasets on the fixture's grid: its two, and a third with other counts and background whose components
    trade PSFs ("extended" takes the 5x5, "points" the 9x9): a third pair of plans."""
    datasets = unpack_datasets(m)
    rs = np.random.RandomState(23)
    third = {k: (v.copy() if not isinstance(v, dict) else dict(v)) for k, v in datasets["o1"].items()}
    third["psf"] = {"extended": datasets["o1"]["psf"]["points"], "points": datasets["o1"]["psf"]["extended"]}
    third["counts"] = rs.poisson(np.clip(datasets["o0"]["counts"] * 0.7 + 0.5, 0, None)).astype(np.float32)
    third["background"] = third["background"] * 1.5
    datasets["o2"] = third
    return datasets


def test_joint_mode_equals_the_per_dataset_loop_and_the_oracle(golden):
    """Joint mode over 3 datasets: the fit loop's joint step IS the per-dataset loop with `accumulate` from the second
    dataset on -- a session's gradient buffers and dataset losses after one epoch equal, bit for bit, what that loop
    leaves (priors that add nothing and a learning rate of zero keep them in place), which in turn is the sum of the
    per-dataset gradients; and a 3-epoch joint fit follows cpu_ref.map_fit_joint."""
    from jolideco_amd import FluxComponents, MAPDeconvolver, PoissonLoss, SpatialFluxComponent, UniformPrior
    from oracle import cpu_ref

    m = golden("mixed_upsampling")
    datasets = _three_datasets(m)
    plain = FluxComponents()
    for name, u in (("extended", 1), ("points", 2)):
        plain[name] = SpatialFluxComponent.from_numpy(flux=m[f"init/{name}"], upsampling_factor=u, prior=UniformPrior())
    session = MAPDeconvolver(n_epochs=1, display_progress=False, device=DEV, fit_mode="joint",
                             learning_rate=0.0).session(datasets, components=plain)
    poisson = PoissonLoss.from_datasets(datasets, _components(m, 1, 2), device=DEV)
    assert not poisson.batchable([0, 1, 2]) and not poisson.batchable_calibrated([0, 1, 2])
    assert not session.batch_joint and not session.batch_joint_calibrated
    fluxes = [st.flux_cur.clone() for st in session.states]  # (exp(theta) as the session's own kernel formed it)
    joint = [torch.zeros_like(f) for f in fluxes]
    losses = torch.zeros(3, device=DEV)
    for i in range(3):
        poisson.fwd_bwd(i, fluxes, losses[i : i + 1], grads=joint, accumulate=i > 0)
    single = [np.zeros(f.shape, np.float64) for f in fluxes]
    for i in range(3):
        own = [torch.zeros_like(f) for f in fluxes]
        value = torch.zeros(1, device=DEV)
        poisson.fwd_bwd(i, fluxes, value, grads=own)
        assert float(value) == float(losses[i])
        for acc, g in zip(single, own):
            acc += g.cpu().numpy()
    for g, ref in zip(joint, single):
        assert rel_linf(g.cpu().numpy(), ref) < 1e-6
    session.epoch()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(session.scalars[:3].cpu().numpy(), losses.cpu().numpy())
    for st, g in zip(session.states, joint):
        np.testing.assert_array_equal(st.grad.cpu().numpy(), g.cpu().numpy())

    res = MAPDeconvolver(n_epochs=3, display_progress=False, device=DEV, fit_mode="joint").run(
        datasets, components=_components(m, 1, 2)
    )
    gmm_o = cpu_ref.GMM.from_numpy(m["gmm/means"], m["gmm/covariances"], m["gmm/weights"], stride=4)
    final, trace = cpu_ref.map_fit_joint(
        datasets, {"extended": m["init/extended"], "points": m["init/points"]},
        {"extended": cpu_ref.GMMPatchPriorRef(gmm_o), "points": cpu_ref.InverseGammaPriorRef(10, 1.5)},
        n_epochs=3, upsampling_factors={"extended": 1, "points": 2},
    )
    for name in ("extended", "points"):
        assert rel_linf(res.components[name].flux_upsampled_numpy, final[name]) < 1e-5, name
    np.testing.assert_allclose(np.asarray(res.trace_loss["total"]), [r["total"] for r in trace], rtol=2e-5)


@pytest.mark.parametrize("fit_mode", ["sequential", "joint"])
def test_replayed_epochs_equal_eager_epochs_bit_for_bit(golden, monkeypatch, fit_mode):
    """JOLIDECO_GRAPH=1 (planned epochs, captured and replayed) against JOLIDECO_GRAPH=0: the same bits."""
    from jolideco_amd import MAPDeconvolver

    m = golden("mixed_upsampling")
    datasets = _three_datasets(m)

    def fit(graph):
        monkeypatch.setenv("JOLIDECO_GRAPH", graph)
        comps = _components(m, 1, 2, generator=torch.Generator().manual_seed(5))
        session = MAPDeconvolver(n_epochs=9, display_progress=False, device=DEV, fit_mode=fit_mode).session(
            datasets, components=comps
        )
        rows = []
        for _ in range(9):
            session.epoch()
            rows.append(session.scalars.clone())
        torch.cuda.synchronize()
        return ([st.flux_cur.cpu().numpy().copy() for st in session.states], torch.stack(rows).cpu().numpy(),
                len(session._graphs), session.graph_policy)

    eager, replayed = fit("0"), fit("1")
    assert eager[2] == 0 and replayed[2] >= 1, (eager[3], replayed[3])
    for a, b in zip(eager[0], replayed[0]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eager[1], replayed[1])


def test_forward_only_call_returns_the_loss_of_the_gradient_call(golden):
    from jolideco_amd import PoissonLoss

    m = golden("mixed_upsampling")
    comps = _components(m, 3, 2)
    poisson = PoissonLoss.from_datasets(unpack_datasets(m), comps, device=DEV)
    fluxes = [c.flux_upsampled.detach().reshape(c.flux_upsampled.shape[-2:]).contiguous().to(DEV) for c in comps.values()]
    with_grad = torch.zeros(2, device=DEV)
    for i in range(2):
        poisson.fwd_bwd(i, fluxes, with_grad[i : i + 1], grads=[torch.zeros_like(f) for f in fluxes])
    forward_only = poisson.evaluate([f[None, None] for f in fluxes])  # (PoissonLoss.evaluate: the trace and validation path)
    assert np.array_equal(with_grad.cpu().numpy(), forward_only.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 5. boundaries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factors,mixed", [((2, 2), False), ((1, 2), True)])
def test_only_different_factors_reach_the_new_kernel(golden, factors, mixed):
    """The kernel timers count the launches: a (2, 2) fit never launches the mixed Poisson kernel (it keeps the entry
    and the results it had), a (1, 2) fit launches nothing else for its Poisson pass."""
    from jolideco_amd import MAPDeconvolver, _hip

    m = golden("mixed_upsampling")
    _hip.profile_enable(4096)
    try:
        MAPDeconvolver(n_epochs=2, display_progress=False, device=DEV).run(
            unpack_datasets(m), components=_components(m, *factors)
        )
    finally:
        prof = _hip.profile_read()
    print({k: v[1] for k, v in prof.items() if v[1]})
    if mixed:
        assert prof["poisson_mixed"][1] >= 2 * (2 + 2) and prof["poisson_fused"][1] == 0  # per epoch: 2 steps + 2 trace rows
    else:
        assert prof["poisson_mixed"][1] == 0 and prof["poisson_fused"][1] > 0


def test_calibration_with_different_factors_is_refused(golden):
    from jolideco_amd import MAPDeconvolver, NPredCalibration, NPredCalibrations

    m = golden("mixed_upsampling")
    cals = NPredCalibrations()
    for name in ("o0", "o1"):
        cals[name] = NPredCalibration(shift_x=0.1, background_norm=1.1)
    with pytest.raises(NotImplementedError, match="calibration together with flux components of different upsampling_factor"):
        MAPDeconvolver(n_epochs=1, display_progress=False, device=DEV).run(
            unpack_datasets(m), components=_components(m, 1, 2), calibrations=cals
        )


def test_shape_mismatch_is_reported_by_the_c_entry():
    """A plan whose grid is not its factor times the counts grid of component 0: -1 (JD_ERR_INVALID) with a message,
    nothing launched."""
    from jolideco_amd import _hip
    from jolideco_amd.ops import ConvPlan

    good, bad = ConvPlan.get(40, 44, 5, 5, DEV, method="direct"), ConvPlan.get(80, 92, 5, 5, DEV, method="direct")
    flux = [torch.ones(40, 44, device=DEV), torch.ones(80, 92, device=DEV)]
    khat = [torch.zeros(2 * p.spectrum_size, device=DEV) for p in (good, bad)]
    small = torch.ones(40, 44, device=DEV)
    loss = torch.zeros(1, device=DEV)
    handles = (ctypes.c_void_p * 2)(good._handle.value, bad._handle.value)
    factors = (ctypes.c_int * 2)(1, 2)
    status = _hip.lib().jd_npred_poisson_mixed_fwd_bwd(
        handles, 2, _hip.ptr_array(flux), _hip.ptr_array(flux), _hip.ptr_array(khat), _hip.ptr(small), _hip.ptr(small),
        0.0, 1e-25, _hip.ptr(loss), None, 0, 1.0, None, factors, _hip.stream_ptr(torch.device(DEV)),
    )
    assert status == -1
    assert b"shape mismatch" in _hip.lib().jd_last_error()
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ConvPlan.npred_poisson_mixed_fwd_bwd([good, bad], [1, 2], flux, flux, khat, small, small, 0.0, loss)
    factors = (ctypes.c_int * 2)(1, 9)
    assert _hip.lib().jd_npred_poisson_mixed_fwd_bwd(
        handles, 2, _hip.ptr_array(flux), _hip.ptr_array(flux), _hip.ptr_array(khat), _hip.ptr(small), _hip.ptr(small),
        0.0, 1e-25, _hip.ptr(loss), None, 0, 1.0, None, factors, _hip.stream_ptr(torch.device(DEV)),
    ) == -1
    assert float(loss) == 0.0

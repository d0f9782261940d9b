"""The sessions that never take a plan in device memory -- a replaced `_optimizer_step`, validation datasets, a sharded joint
step -- run through the same epoch body as every other (`FitSession._enqueue_epoch`) with host scalars.  Each must give, BIT
FOR BIT, the plain by-value fit (JOLIDECO_STEP_SCALARS=host) of the same inputs: the anchor-B shape (48 x 40, three
observations, a K = 4 GMM prior at stride 4), 5 epochs, joint and sequential.  A component under `UniformPrior` gets no launch
at all: its slot must read exactly 0.0 after every epoch."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_EPOCHS = 5
SHAPE = (48, 40)


@contextlib.contextmanager
def _environment(**values):
    """JOLIDECO_* variables set (None: unset) for the time a session is built and run."""
    saved = {key: os.environ.get(key) for key in values}
    try:
        for key, value in values.items():
            os.environ.pop(key, None)
            if value is not None:
                os.environ[key] = value
        yield
    finally:
        for key, value in saved.items():
            os.environ.pop(key, None)
            if value is not None:
                os.environ[key] = value


def build(uniform=False):
    """(datasets, the validation dataset, components) of the fit; ``uniform``: a second component under `UniformPrior`."""
    from jolideco_amd import FluxComponents, GMMPatchPrior, SpatialFluxComponent, UniformPrior
    from jolideco_amd.data import point_source_gauss_psf, synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    rs = np.random.RandomState(11)
    datasets = {f"obs-{i}": point_source_gauss_psf(shape=SHAPE, sigma_psf=2 + i, random_state=rs) for i in range(4)}
    for d in datasets.values():
        d.pop("flux")
    validation = {"validation": datasets.pop("obs-3")}
    flux_init = rs.gamma(30, size=SHAPE)
    means, covs, weights = synthetic_gmm(4, 64, seed=2)
    gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))
    comps = FluxComponents()
    comps["flux"] = SpatialFluxComponent.from_numpy(flux=flux_init, prior=GMMPatchPrior(gmm=gmm, generator=torch.Generator().manual_seed(5)))
    if uniform:
        comps["flat"] = SpatialFluxComponent.from_numpy(flux=0.1 * flux_init, prior=UniformPrior())
    return datasets, validation, comps


def fit(fit_mode, uniform=False, hook=False, validation=False, dist=None, optimizer_type="adam"):
    """Run the fit; returns {"images": fluxes + thetas, "scalars": one row per epoch, "steps": what the hook saw, "session"}."""
    from jolideco_amd import MAPDeconvolver

    datasets, datasets_validation, comps = build(uniform)
    deco = MAPDeconvolver(n_epochs=N_EPOCHS, display_progress=False, device=DEV, fit_mode=fit_mode, optimizer_type=optimizer_type)
    steps = []
    if hook:
        real = deco._optimizer_step

        def recording_step(states, step):
            steps.append(step)
            real(states, step)

        deco._optimizer_step = recording_step
    session = deco.session(datasets, datasets_validation if validation else None, components=comps, dist=dist)
    rows = []
    for _ in range(N_EPOCHS):
        session.epoch()
        rows.append(session.scalars.clone())
    torch.cuda.synchronize()
    images = [st.flux_cur.cpu().numpy().copy() for st in session.states] + [st.theta.cpu().numpy().copy() for st in session.states]
    return {"images": images, "scalars": torch.stack(rows).cpu().numpy(), "steps": steps, "session": session}


@functools.lru_cache(maxsize=None)
def plain(fit_mode, uniform):
    """The by-value fit every session here is held to (computed once per form, never changed)."""
    with _environment(JOLIDECO_STEP_SCALARS="host", JOLIDECO_GRAPH="0"):
        result = fit(fit_mode, uniform)
    result.pop("session")
    return result


def _default_environment():
    return _environment(JOLIDECO_STEP_SCALARS=None, JOLIDECO_GRAPH=None, JOLIDECO_PRIOR_OVERLAP=None)


def _assert_same_fit(got, want, n_slots=None):
    for a, b in zip(got["images"], want["images"]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got["scalars"][:, :n_slots], want["scalars"])
    assert np.all(np.isfinite(got["scalars"]))


def _assert_uniform_slot_is_zero(result):
    n_d = result["session"].n_d
    column = result["scalars"][:, n_d + 1]
    assert column.shape == (N_EPOCHS,) and np.all(column == 0.0) and not np.any(np.signbit(column))
    assert np.all(result["scalars"][:, n_d] != 0.0)  # (the GMM prior beside it does write its slot)


@pytest.mark.parametrize("uniform", [False, True], ids=["gmm", "gmm+uniform"])
@pytest.mark.parametrize("fit_mode", ["joint", "sequential"])
def test_a_session_with_a_replaced_optimizer_step(fit_mode, uniform):
    with _default_environment():
        hooked = fit(fit_mode, uniform, hook=True)
    n_steps = N_EPOCHS * (1 if fit_mode == "joint" else 3)
    assert hooked["steps"] == list(range(1, n_steps + 1)) and hooked["session"].step == n_steps
    assert not hooked["session"]._planned_capable() and not hooked["session"]._graphs
    _assert_same_fit(hooked, plain(fit_mode, uniform))
    if uniform:
        _assert_uniform_slot_is_zero(hooked)


@pytest.mark.parametrize("fit_mode", ["joint", "sequential"])
def test_a_session_with_a_validation_dataset(fit_mode):
    with _default_environment():
        validated = fit(fit_mode, validation=True)
    session = validated["session"]
    assert session.n_val == 1 and validated["scalars"].shape == (N_EPOCHS, session.n_d + session.n_c + 1)
    _assert_same_fit(validated, plain(fit_mode, False), n_slots=session.n_d + session.n_c)
    assert np.all(np.isfinite(validated["scalars"][:, -1])) and np.all(validated["scalars"][:, -1] != 0.0)


@pytest.mark.parametrize("uniform", [False, True], ids=["gmm", "gmm+uniform"])
@pytest.mark.parametrize("fit_mode", ["joint", "sequential"])
def test_a_one_rank_dry_run_sharded_session(fit_mode, uniform):
    """One rank that takes the sharded route without a process group: `DistContext(0, 1, dry_run=True)` with the
    collectives forced -- the band plan, the band sum with the optimizer step, the rank-ordered sum in its dry-run form."""
    from jolideco_amd.distributed import DistContext

    dist = DistContext(rank=0, world_size=1, dry_run=True, force_collectives=True)
    assert dist.sharded
    with _default_environment():
        sharded = fit(fit_mode, uniform, dist=dist)
    session = sharded["session"]
    assert bool(session.band_plan) == (fit_mode == "joint") and not session._planned_capable()
    _assert_same_fit(sharded, plain(fit_mode, uniform))
    if uniform:
        _assert_uniform_slot_is_zero(sharded)

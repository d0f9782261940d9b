"""CPU: the GMM patch prior on 16x16 patches (256 features) against tests/golden/gmm16.npz, generated from the LIVE
reference by tools/make_golden_gmm16.py: the oracle reproduces the fixture, the C ABI takes D = 256 (and only 64 and
256), the prior's abilities are per instance, (de)serialisation."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import rel_linf, unpack_datasets
from tools import gmm16_cases as cases

from jolideco_amd import GMMPatchPrior
from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
from jolideco_amd.utils.norms import ASinhImageNorm
from oracle import cpu_ref


def _model(arrays, stride=cases.STRIDE):
    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


def test_fixture_mixtures_are_the_ones_rebuilt_here(golden):
    g = golden("gmm16")
    assert (int(g["K"]), int(g["seed"]), int(g["stride"])) == (cases.K, cases.SEED, cases.STRIDE)
    assert (int(g["fit/K"]), int(g["fit/seed"])) == (cases.FIT_K, cases.FIT_GMM_SEED)
    arrays = cases.synthetic_mixture(cases.K, cases.SEED)
    assert arrays[1].shape == (cases.K, 256, 256)
    assert cases.mixture_checksum(arrays) == pytest.approx(float(g["gmm/checksum"]), rel=1e-13)
    assert cases.mixture_checksum(cases.synthetic_mixture(cases.FIT_K, cases.FIT_GMM_SEED)) == pytest.approx(
        float(g["fit/gmm/checksum"]), rel=1e-13)
    assert np.array_equal(g["flux"], cases.fixture_flux()) and g["flux"][cases.FILTERED_PIXEL] == -2e5


@pytest.mark.parametrize("marginalize", [False, True])
@pytest.mark.parametrize("normed", [False, True])
def test_oracle_reproduces_the_reference_prior(golden, normed, marginalize):
    """oracle/cpu_ref on [asinh of] the flux = the reference's GMMPatchPrior on 16x16 patches (bit for bit when the
    fixture was generated; another torch build may differ at rounding).  Exactly one patch is filtered in the bare case;
    under the norm the -2e5 pixel maps above -1e5 and every patch counts, as in the reference."""
    g = golden("gmm16")
    arrays = cases.synthetic_mixture(cases.K, cases.SEED)
    norm = ASinhImageNorm(**cases.ASINH) if normed else None
    o = cases.oracle(g["flux"], arrays, cases.STRIDE, None, marginalize, norm=norm)
    assert int((~o["keep"]).sum()) == (0 if normed else 1) and o["keep"].size == 30
    scale = cases.prior_scale(cases.SHAPE, cases.STRIDE)
    tag = f"{'asinh' if normed else 'bare'}/{'lse' if marginalize else 'max'}"
    np.testing.assert_allclose(o["total"] * scale, float(g[f"{tag}/value"]), rtol=2e-6)
    assert rel_linf(o["grad"] * scale, g[f"{tag}/grad"]) < 1e-5
    assert np.abs(g[f"{tag}/grad"]).max() > 0
    if not normed:  # the filtered patch contributes nothing: the pixels only it covers have no gradient
        assert np.all(g[f"{tag}/grad"][:8, :8] == 0) and not o["keep"][0]


def test_oracle_reproduces_the_reference_log_prob(golden):
    g = golden("gmm16")
    gmm = cpu_ref.GMM.from_numpy(*cases.synthetic_mixture(cases.K, cases.SEED), stride=cases.STRIDE)
    x = cases.mean_free_patches(cases.fixture_flux(filtered=False), cases.STRIDE)
    assert x.shape == (30, 256)
    np.testing.assert_allclose(cpu_ref.gmm_log_prob(torch.from_numpy(x), gmm).numpy(), g["log_prob"], rtol=2e-6)


def test_oracle_reproduces_the_reference_fit(golden):
    g = golden("gmm16")
    gmm = cpu_ref.GMM.from_numpy(*cases.synthetic_mixture(cases.FIT_K, cases.FIT_GMM_SEED), stride=cases.STRIDE)
    final, trace = cpu_ref.map_fit_sequential(
        unpack_datasets(g, "fit/data/"), {"flux": g["fit/flux_init"]}, {"flux": cpu_ref.GMMPatchPriorRef(gmm)},
        n_epochs=cases.FIT_EPOCHS,
    )
    assert rel_linf(final["flux"], g["fit/flux_final"]) < 1e-5
    np.testing.assert_allclose([row["total"] for row in trace], g["fit/trace/total"], rtol=2e-5)


def test_cabi_takes_64_and_256_features_only():
    """jd_gmm_create: D = 16 and D = 128 are refused as invalid, naming what is supported; D = 256 passes the argument
    checks (without a GPU it then fails in the HIP runtime, which is a different status)."""
    from jolideco_amd import _hip

    lib = _hip.lib()
    handle = ctypes.c_void_p()
    small = (ctypes.c_float * 4)()
    fp = ctypes.cast(small, ctypes.POINTER(ctypes.c_float))
    for d in (16, 128):
        assert lib.jd_gmm_create(1, d, fp, fp, fp, fp, ctypes.byref(handle)) == -1
        msg = lib.jd_last_error()
        assert b"D = 64" in msg and b"D = 256" in msg and str(d).encode() in msg
    as_fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    pc = np.ascontiguousarray(np.eye(256, dtype=np.float32)[None])
    mp, ck, pw = np.zeros((1, 256), np.float32), np.zeros(1, np.float32), np.ones(256, np.float32)
    rc = lib.jd_gmm_create(1, 256, as_fp(pc), as_fp(mp), as_fp(ck), as_fp(pw), ctypes.byref(handle))
    assert rc != -1, lib.jd_last_error()
    if rc == 0:
        assert lib.jd_gmm_is_triangular(handle) == 1
        assert lib.jd_gmm_destroy(handle) == 0
    else:
        assert b"D = 64" not in lib.jd_last_error()


def test_abilities_are_per_instance():
    gmm16 = _model(cases.synthetic_mixture(2, 5))
    means, covs, weights = cpu_ref.synthetic_gmm(2, 64, seed=5)
    gmm8 = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))
    p16, p8 = GMMPatchPrior(gmm=gmm16), GMMPatchPrior(gmm=gmm8)
    assert p16.patch_shape == (16, 16) and p16.stride == 8 and p16.overlap == 8
    assert (p16.supports_fused_step, p16.supports_phases, p16.shardable) == (False, False, False)
    assert (p8.supports_fused_step, p8.supports_phases, p8.shardable) == (True, True, True)
    assert p16.log_like_weight == 64 / 256 and p16.n_patch_rows((48, 56)) == 5
    # cycle-spin draws: patch_shape // 4 = +-4, and the same numbers one by one or an epoch at a time
    a, b = torch.Generator(device="cpu"), torch.Generator(device="cpu")
    one = GMMPatchPrior(gmm=gmm16, generator=a)
    many = GMMPatchPrior(gmm=gmm16, generator=b)
    draws = [one.draw_shifts() for _ in range(64)]
    assert draws == many.draw_shifts_many(64)
    flat = np.array(draws).ravel()
    assert flat.min() == -4 and flat.max() == 4
    for kwargs in ({"jitter": True}, {"cycle_spin_subpix": True}):
        with pytest.raises(NotImplementedError):
            GMMPatchPrior(gmm=gmm16, **kwargs)


def test_sharded_sessions_take_the_unsharded_route_for_a_16x16_prior():
    """`FitSession` shards the patch rows of `shardable` priors only; every other prior is evaluated whole on rank 0 and
    reaches the other ranks through the all-reduce of the gradient.  A 16x16 prior is of the second kind: its rows are
    never split, whatever the session's world size.

    What this test shows and what it does not: on stand-ins for the session it shows that the rows of a 16x16 prior are
    never handed to `shard_range` and that its gather does not take the optimizer step.  It does not run two ranks, so it
    does not show the evaluation on rank 0 alone and the all-reduce that carries it to the others; that route is the one
    the element-wise priors of every sharded fit already take (tests/test_gpu_distributed.py, tests/test_distributed_gloo.py)."""
    from jolideco_amd.core import FitSession

    class Dist:
        sharded = True

        def shard_range(self, n, shares):
            raise AssertionError("a 16x16 prior must not be sharded")

    class Stub:
        joint, dist, prior_shares = True, Dist(), None

    class State:
        shape, frozen = (48, 56), False

    p16 = GMMPatchPrior(gmm=_model(cases.synthetic_mixture(2, 5)))
    assert FitSession._prior_rows(Stub(), p16, State()) is None

    # single process: no optimizer step in the prior's gather (the 8x8 prior of the same session takes it)
    class Single:
        sharded = False

    class Config:
        pass

    class One:
        fuse_optimizer_step, dist, cfg = True, Single(), Config()

    means, covs, weights = cpu_ref.synthetic_gmm(2, 64, seed=5)
    p8 = GMMPatchPrior(gmm=GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4)))
    assert not FitSession._fuse_step(One(), State(), p16) and FitSession._fuse_step(One(), State(), p8)


def test_to_dict_from_dict_round_trip(tmp_path, monkeypatch):
    """A 16x16 mixture of the user's library: the prior's header rebuilds the same prior (the mixture by name)."""
    gmm16 = _model(cases.synthetic_mixture(2, 5))
    custom = GMMPatchPrior(gmm=gmm16).to_dict()
    assert custom["stride"] == 8 and custom["gmm"] == {"type": "custom", "n_components": 2, "n_features": 256}
    path = tmp_path / "gmm16.fits"
    gmm16.write(path)
    index = {"synthetic-16x16": {"filename": str(path), "format": "table"}}
    (tmp_path / "jolideco-gmm-library-index.json").write_text(json.dumps(index))
    monkeypatch.setenv("JOLIDECO_GMM_LIBRARY", str(tmp_path))
    prior = GMMPatchPrior(gmm=GaussianMixtureModel.from_registry("synthetic-16x16"), marginalize=True,
                          norm=ASinhImageNorm(**cases.ASINH))
    data = prior.to_dict()
    assert data["gmm"] == {"type": "synthetic-16x16"} and data["marginalize"] is True and data["stride"] == 8
    back = GMMPatchPrior.from_dict(json.loads(json.dumps(data)))
    assert back.patch_shape == (16, 16) and back.stride == 8 and back.marginalize and back.to_dict() == data
    assert (back.supports_fused_step, back.supports_phases, back.shardable) == (False, False, False)
    np.testing.assert_allclose(back.gmm.covariances_numpy, gmm16.covariances_numpy, rtol=1e-6)

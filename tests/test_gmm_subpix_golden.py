"""CPU: the GMM patch prior with a sub-pixel cycle spin (`SubpixelGMMPatchPrior`, the reference's `cycle_spin_subpix=True`) -- the oracle of
tests/gmm_subpix_cases.py against tests/golden/gmm_subpix.npz (generated from the live reference by
tools/make_golden_gmm_subpix.py), the draw order, what the option switches off, and the written formats."""
import json

import numpy as np
import pytest
import torch

import gmm_subpix_cases as cases
from conftest import REPO, unpack_datasets
from oracle import cpu_ref


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("gmm_subpix")


def _model(arrays, stride=4):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


def _small_gmm():
    return _model(cpu_ref.synthetic_gmm(2, 64, seed=0))


def _prior(**kwargs):
    from jolideco_amd import SubpixelGMMPatchPrior

    return SubpixelGMMPatchPrior(gmm=_small_gmm(), **kwargs)


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_reproduces_the_fixture(golden, fixture):
    """The float32 oracle on the fixture's replayed draws: value and gradient of the live reference within 1e-6 (relative;
    the gradient in L-infinity) -- what the generator asserted, held here without the reference."""
    from jolideco_amd.utils.norms import ASinhImageNorm

    arrays = cases.fixture_gmm(golden)
    for tag in fixture["tags"]:
        index = int(fixture[f"{tag}/index"])
        shape, stride, _, _ = cases.CASES[index]
        roll = tuple(int(v) for v in fixture[f"{tag}/roll"])
        roll = None if roll == (-99, -99) else roll
        offsets = tuple(float(v) for v in fixture[f"{tag}/offsets"])
        norm = ASinhImageNorm(alpha=3.0, beta=40.0) if tag.endswith("asinh") else None
        total, grad, _, _ = cases.oracle(cases.case_flux(index), norm, arrays, stride, roll, offsets, tag.endswith("lse"), np.float32)
        scale = stride**2 / 64.0 / (shape[0] * shape[1])
        value = float(fixture[f"{tag}/value"])
        assert abs(total * scale - value) <= 1e-6 * abs(value), tag
        assert cases.rel_err(grad * scale, fixture[f"{tag}/grad"]) <= 1e-6, tag


def test_fixture_draws_are_the_generator_replayed(fixture):
    """roll (rows first), then x0, then y0 -- `SubpixelGMMPatchPrior.draw_shifts` from the fixture's seeds gives the fixture's draws"""
    for tag in fixture["tags"]:
        cycle_spin = not tag.endswith("no_roll")
        prior = _prior(cycle_spin=cycle_spin, generator=torch.Generator("cpu").manual_seed(int(fixture[f"{tag}/seed"])))
        roll, offsets = prior.draw_shifts()
        assert (roll is None) == (not cycle_spin)
        assert ((-99, -99) if roll is None else roll) == tuple(int(v) for v in fixture[f"{tag}/roll"])
        assert offsets == tuple(float(v) for v in fixture[f"{tag}/offsets"])
        assert prior.last_shifts == (roll, offsets)


def test_near_ties_are_rare_in_every_case(golden):
    """Max mode: patches whose two best float64 log-likelihoods are closer than NEAR_TIE number at most 1 % of the patches
    of every case -- the condition under which the GPU test leaves them out of its gradient comparison."""
    for table, rows in ((64, cases.CASES), (256, cases.CASES_256)):
        for index in range(len(rows)):
            margin = cases.cached_oracle(golden, index, False, np.float64, table=table)[3]
            ties = int((margin < cases.NEAR_TIE).sum())
            print(f"D = {table} case {index} {rows[index][0]}: {ties} near ties of {margin.size} patches, min margin {margin.min():.3g}")
            assert ties <= 0.01 * margin.size, (table, index)


def test_seam_and_tile_layout_of_the_large_case():
    """The (72, 100) case spans more than one tile both ways; one roll puts the seam strictly inside a tile, one on a tile edge"""
    ty, tx = cases.TILE
    large = [c for c in cases.CASES if c[0] == (72, 100)]
    assert len(large) == 2 and 72 > ty and 100 > tx
    seams = [((72 - roll[0]) % 72, (100 - roll[1]) % 100) for _, _, roll, _ in large]
    assert seams[0][0] % ty != 0 and seams[0][1] % tx != 0
    assert seams[1][0] % ty == 0 and seams[1][1] % tx == 0 and seams[1] != (0, 0)
    text = (REPO / "jolideco_amd" / "csrc" / "gmm_subpix.hip").read_text()
    assert f"GS_TX = {tx}, GS_TY = {ty}" in text  # (the tile shape the case table was laid out for)


# ------------------------------------------------------------------------------------------------ draws
def test_draw_order_against_a_replay_of_the_generator():
    from jolideco_amd import GMMPatchPrior

    for cycle_spin in (True, False):
        prior = _prior(cycle_spin=cycle_spin, generator=torch.Generator("cpu").manual_seed(41))
        replay = torch.Generator("cpu").manual_seed(41)
        for _ in range(4):
            roll = None
            if cycle_spin:
                rows = torch.randint(-2, 3, (1,), generator=replay)
                cols = torch.randint(-2, 3, (1,), generator=replay)
                roll = (int(rows), int(cols))
            x0 = torch.rand(1, generator=replay) - 0.5
            y0 = torch.rand(1, generator=replay) - 0.5
            drawn = prior.draw_shifts()
            assert drawn == (roll, (float(x0), float(y0))) == prior.last_shifts
            assert all(isinstance(v, float) and np.float32(v) == v for v in drawn[1])
    one = _prior(generator=torch.Generator("cpu").manual_seed(7))
    many = _prior(generator=torch.Generator("cpu").manual_seed(7))
    draws = [one.draw_shifts() for _ in range(9)]
    assert many.draw_shifts_many(9) == draws and many.last_shifts == draws[-1]
    assert torch.equal(one.generator.get_state(), many.generator.get_state())
    # default generators: the reference's default seed, like the oracle prior's
    ours, theirs = _prior(), torch.Generator("cpu")
    assert [ours.draw_shifts() for _ in range(3)] == [cases.draw(theirs) for _ in range(3)]
    # with the flag off nothing changes: plain pairs, batched draws
    plain = GMMPatchPrior(gmm=_small_gmm(), generator=torch.Generator("cpu").manual_seed(7))
    assert plain.shift_kind == "roll" and isinstance(plain.draw_shifts()[0], int)


# ------------------------------------------------------------------------------------------------ what it switches
def test_constructor_flags_and_refusals():
    import jolideco_amd as jd
    from jolideco_amd.priors import PRIOR_REGISTRY
    from jolideco_amd.priors.patches import MultiScalePrior

    prior = _prior()
    assert prior.cycle_spin_subpix is True and prior.jitter is False and prior.shift_kind == "roll+subpixel"
    assert (prior.shardable, prior.supports_fused_step, prior.supports_phases) == (False, False, False)
    plain = jd.GMMPatchPrior(gmm=_small_gmm())
    assert plain.cycle_spin_subpix is False and (plain.shardable, plain.supports_fused_step, plain.supports_phases) == (True, True, True)
    with pytest.raises(NotImplementedError, match="jitter"):
        jd.GMMPatchPrior(gmm=_small_gmm(), jitter=True)
    with pytest.raises(NotImplementedError, match="jitter"):
        jd.SubpixelGMMPatchPrior(gmm=_small_gmm(), jitter=True)
    # the plain class keeps refusing the switch and names the class that has it; the subclass is that switch
    with pytest.raises(NotImplementedError, match="cycle_spin_subpix .* SubpixelGMMPatchPrior"):
        jd.GMMPatchPrior(gmm=_small_gmm(), cycle_spin_subpix=True)
    with pytest.raises(ValueError, match="cycle_spin_subpix=True"):
        jd.SubpixelGMMPatchPrior(gmm=_small_gmm(), cycle_spin_subpix=False)
    assert isinstance(prior, jd.GMMPatchPrior) and jd.SubpixelGMMPatchPrior(gmm=_small_gmm(), cycle_spin_subpix=True).cycle_spin_subpix
    assert jd.SubpixelGMMPatchPrior not in PRIOR_REGISTRY.values() and prior.to_dict()["type"] == "gmm-patches"
    with pytest.raises(NotImplementedError, match="cycle_spin_subpix"):
        prior.check_hessian_ones()
    with pytest.raises(NotImplementedError, match="cycle_spin_subpix"):
        prior.hessian_ones(torch.ones((1, 1, 16, 16)))
    plain.check_hessian_ones()
    with pytest.raises(NotImplementedError, match="cycle_spin_subpix"):
        MultiScalePrior(prior)
    MultiScalePrior(plain)
    with pytest.raises(NotImplementedError, match="fused optimizer step"):
        prior.device_fwd_bwd_step(torch.ones((16, 16)), None, 1.0, None)
    with pytest.raises(ValueError, match="pair"):
        prior._split_shifts((1, 2))
    assert prior._split_shifts(((1, 2), (0.25, -0.5))) == ((1, 2), (0.25, -0.5))
    assert plain._split_shifts((1, 2)) == ((1, 2), None)


def test_to_dict_and_from_dict(tmp_path, monkeypatch):
    import jolideco_amd as jd
    from jolideco_amd.priors import Prior

    gmm = _gmm_library(tmp_path, monkeypatch)
    prior = jd.SubpixelGMMPatchPrior(gmm=gmm, cycle_spin=False)
    data = prior.to_dict()
    assert data["cycle_spin_subpix"] is True and data["jitter"] is False and data["cycle_spin"] is False
    back = Prior.from_dict(data)
    assert type(back) is jd.SubpixelGMMPatchPrior and back.cycle_spin_subpix is True and back.cycle_spin is False
    assert back.to_dict() == data
    plain = jd.GMMPatchPrior(gmm=gmm)
    assert plain.to_dict()["cycle_spin_subpix"] is False and type(Prior.from_dict(plain.to_dict())) is jd.GMMPatchPrior
    assert type(jd.SubpixelGMMPatchPrior.from_dict({k: v for k, v in data.items() if k != "type"})) is jd.SubpixelGMMPatchPrior


def _gmm_library(tmp_path, monkeypatch):
    """A user's GMM library directory with one synthetic model registered as "zoran-weiss" (tests/test_io_formats.py)"""
    from jolideco_amd.priors.patches import GaussianMixtureModel

    arrays = tuple(a.astype(np.float32).astype(np.float64) for a in cpu_ref.synthetic_gmm(3, 64, seed=11, zero_means=False))
    _model(arrays).write(tmp_path / "zw.fits")
    index = {"zoran-weiss": {"filename": "$JOLIDECO_GMM_LIBRARY/zw.fits", "format": "table"}}
    (tmp_path / "jolideco-gmm-library-index.json").write_text(json.dumps(index))
    monkeypatch.setenv("JOLIDECO_GMM_LIBRARY", str(tmp_path))
    return GaussianMixtureModel.from_registry("zoran-weiss")


@pytest.mark.parametrize("format", ["fits", "yaml"])
def test_written_formats_round_trip(format, tmp_path, monkeypatch):
    """The flag travels through the FITS header (PSUBSPIN) and YAML"""
    import jolideco_amd as jd
    from jolideco_amd.utils.io._fitsfile import read_fits

    gmm = _gmm_library(tmp_path, monkeypatch)
    for flag in (True, False):
        component = jd.SpatialFluxComponent(flux_upsampled=torch.ones((1, 1, 16, 16)), prior=(jd.SubpixelGMMPatchPrior if flag else jd.GMMPatchPrior)(gmm=gmm))
        filename = tmp_path / f"subpix_{flag}.{format}"
        component.write(filename=filename, format=format)
        back = jd.SpatialFluxComponent.read(filename=filename, format=format)
        assert type(back.prior) is (jd.SubpixelGMMPatchPrior if flag else jd.GMMPatchPrior) and back.prior.cycle_spin_subpix is flag
        assert back.prior.to_dict() == component.prior.to_dict()
        if format == "fits":
            header = [hdu.header for hdu in read_fits(filename) if "PTYPE" in hdu.header][0]
            assert header["PSUBSPIN"] is flag and header["PJITTER"] is False
        else:
            assert f"cycle_spin_subpix: {'true' if flag else 'false'}" in filename.read_text()


# ------------------------------------------------------------------------------------------------ the session
def test_session_flags():
    """A session with such a prior runs by-value epochs only, evaluates the prior whole (no shard, no step in its gather),
    and refuses `compute_error` -- on stand-ins for the session and in `FitSession.__init__` up to its refusals (they come
    before anything touches a device).  With the flag off a session is today's."""
    import jolideco_amd as jd
    from jolideco_amd.core import FitSession
    from jolideco_amd.distributed import DistContext

    session = FitSession.__new__(FitSession)
    session.has_sparse, session.has_multiscale, session.has_subpix_patches = False, False, True
    assert session._planned_capable() is False

    class Dist:
        sharded = True

        def shard_range(self, n, shares):
            raise AssertionError("a prior with a sub-pixel cycle spin must not be sharded")

    class Stub:
        joint, dist, prior_shares = True, Dist(), None

    class State:
        shape, frozen = (32, 32), False

    class Single:
        sharded = False

    class Config:
        pass

    class One:
        fuse_optimizer_step, dist, cfg = True, Single(), Config()

    spun, plain = _prior(), jd.GMMPatchPrior(gmm=_small_gmm())
    assert FitSession._prior_rows(Stub(), spun, State()) is None
    assert not FitSession._fuse_step(One(), State(), spun) and FitSession._fuse_step(One(), State(), plain)

    datasets = {"o0": {key: np.ones((32, 32), dtype=np.float32) for key in ("counts", "exposure", "background")}}
    datasets["o0"]["psf"] = np.ones((3, 3), dtype=np.float32) / 9
    comps = jd.FluxComponents()
    comps["flux"] = jd.SpatialFluxComponent.from_numpy(flux=np.full((32, 32), 3.0), prior=spun)
    with pytest.raises(NotImplementedError, match="compute_error=True .* cycle_spin_subpix"):
        FitSession(jd.MAPDeconvolver(n_epochs=1, device="cuda:0", compute_error=True), datasets, None, comps, DistContext.current())


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_of_the_entry():
    """The new symbol is declared, exported and bound; a null handle, flux or value returns JD_ERR_INVALID with a message"""
    from jolideco_amd import _hip

    name = "jd_gmm_prior_subpix_fwd_bwd"
    header = (REPO / "include" / "jolideco_hip.h").read_text()
    assert f"int {name}(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y, int shift_x," in header
    assert "const int* shift_dev, const float* offset_dev, void* stream);" in header
    lib = _hip.lib()
    assert name in _hip.EXPORTS and hasattr(lib, name) and len(_hip.EXPORTS[name][1]) == 19
    assert lib.jd_gmm_prior_subpix_fwd_bwd(None, None, 16, 16, 4, 0, 0, 0.0, 0.0, 0, 1.0, None, 0, 0.0, None, None, None, None, None) == -1
    assert b"jd_gmm_prior_subpix_fwd_bwd: null argument" in lib.jd_last_error()


def test_fit_fixture_layout(fixture):
    datasets = unpack_datasets(fixture, "fit/data/")
    assert sorted(datasets) == ["o0", "o1"] and datasets["o0"]["counts"].shape == cases.FIT_SHAPE
    assert fixture["fit/flux_init"].shape == fixture["fit/flux_final"].shape == cases.FIT_SHAPE
    assert len(fixture["fit/trace/total"]) == cases.FIT_EPOCHS

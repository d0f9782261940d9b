"""CPU: the GMM patch prior with a jittered patch grid (`JitteredGMMPatchPrior`, the reference's `jitter=True`) -- the oracle
of tests/gmm_jitter_cases.py against tests/golden/gmm_jitter.npz (generated from the live reference by
tools/make_golden_gmm_jitter.py), the draw order, the shapes it refuses, what the option switches off, and the written
formats."""
import json

import numpy as np
import pytest
import torch

import gmm_jitter_cases as cases
from conftest import REPO, unpack_datasets
from oracle import cpu_ref
from tools import gmm16_cases


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("gmm_jitter")


def _model(arrays, stride=4):
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))


def _small_gmm(features=64, stride=4):
    return _model(cpu_ref.synthetic_gmm(2, features, seed=0), stride=stride)


def _prior(**kwargs):
    from jolideco_amd import JitteredGMMPatchPrior

    return JitteredGMMPatchPrior(gmm=kwargs.pop("gmm", None) or _small_gmm(), **kwargs)


def _roll(fixture, tag):
    roll = tuple(int(v) for v in fixture[f"{tag}/roll"])
    return None if roll == (-99, -99) else roll


# ------------------------------------------------------------------------------------------------ the oracle and the draws
def test_draws_replay_the_reference_and_the_oracle_reproduces_the_fixture(golden, fixture):
    """`JitteredGMMPatchPrior.draw_shifts(shape)` from the fixture's seed gives the draws of the live reference (two roll
    draws, then the columns' jitter, then the rows'), and the float32 oracle on them gives its value and gradient within 1e-6
    (relative; the gradient in L-infinity) -- what the generator asserted, held here without the reference."""
    from jolideco_amd.utils.norms import ASinhImageNorm

    arrays64 = cases.fixture_gmm(golden)
    assert len(fixture["tags"]) == 20
    for tag in fixture["tags"]:
        table, index = int(fixture[f"{tag}/table"]), int(fixture[f"{tag}/index"])
        rows, patch, _ = cases.table_of(table)
        shape, stride, _ = rows[index]
        cycle_spin = not tag.endswith("no_roll")
        gmm = _small_gmm() if table == 64 else _small_gmm(256, 8)
        prior = _prior(gmm=gmm, stride=stride, cycle_spin=cycle_spin,
                       generator=torch.Generator("cpu").manual_seed(int(fixture[f"{tag}/seed"])))
        roll, (jitter_x, jitter_y) = drawn = prior.draw_shifts(shape)
        assert prior.last_shifts is drawn and (roll is None) == (not cycle_spin) and roll == _roll(fixture, tag), tag
        assert jitter_x.dtype == jitter_y.dtype == torch.int64
        assert np.array_equal(jitter_y.numpy(), fixture[f"{tag}/jitter_y"]) and np.array_equal(jitter_x.numpy(), fixture[f"{tag}/jitter_x"]), tag
        norm = ASinhImageNorm(alpha=3.0, beta=40.0) if tag.endswith("asinh") else None
        arrays, meta = (arrays64, cases.GMM_META_STRIDE) if table == 64 else (cases.mixture256(), gmm16_cases.STRIDE)
        total, grad, _, _ = cases.oracle(cases.case_flux(index, table), norm, arrays, patch, stride, roll,
                                         (jitter_y.numpy(), jitter_x.numpy()), tag.endswith("lse"), np.float32, meta_stride=meta)
        scale = stride**2 / float(patch * patch) / (shape[0] * shape[1])
        value = float(fixture[f"{tag}/value"])
        assert abs(total * scale - value) <= 1e-6 * abs(value), tag
        assert cases.rel_err(grad * scale, fixture[f"{tag}/grad"]) <= 1e-6, tag


def test_draw_order_against_a_replay_of_the_generator():
    """Two roll draws (rows first), then `randint(-overlap, overlap + 1, (n_x,))`, then `(n_y,)` -- also at overlap 0, where
    the draws are all 0 and the generator still advances"""
    for stride, shape in ((4, (40, 44)), (8, (24, 27))):
        overlap = 8 - stride
        for cycle_spin in (True, False):
            prior = _prior(stride=stride, cycle_spin=cycle_spin, generator=torch.Generator("cpu").manual_seed(41))
            replay = torch.Generator("cpu").manual_seed(41)
            n_y, n_x = prior.check_shape(shape)
            assert (n_y, n_x) == tuple(len(b) for b in cases.grid(shape, 8, stride))
            for _ in range(3):
                roll = None
                if cycle_spin:
                    rows = torch.randint(-2, 3, (1,), generator=replay)
                    cols = torch.randint(-2, 3, (1,), generator=replay)
                    roll = (int(rows), int(cols))
                jx = torch.randint(-overlap, overlap + 1, (n_x,), generator=replay)
                jy = torch.randint(-overlap, overlap + 1, (n_y,), generator=replay)
                drawn = prior.draw_shifts(shape)
                assert drawn[0] == roll and torch.equal(drawn[1][0], jx) and torch.equal(drawn[1][1], jy)
                assert overlap or (not jx.any() and not jy.any())
            assert torch.equal(prior.generator.get_state(), replay.get_state())
    prior = _prior()
    with pytest.raises(ValueError, match="draw_shifts\\(shape\\)"):
        prior.draw_shifts()
    # default generators: the reference's default seed, like the oracle prior's
    ours, theirs = _prior(), torch.Generator("cpu")
    for _ in range(2):
        got, want = ours.draw_shifts((32, 32)), cases.draw(theirs, (32, 32))
        assert got[0] == want[0] and np.array_equal(got[1][1].numpy(), want[1][0]) and np.array_equal(got[1][0].numpy(), want[1][1])
    # an unsafe shape raises before the generator advances
    state = ours.generator.get_state()
    with pytest.raises(ValueError):
        ours.draw_shifts((37, 41))
    assert torch.equal(ours.generator.get_state(), state)


def test_near_ties_are_rare_in_every_case(golden):
    """Max mode: patches whose two best float64 log-likelihoods are closer than NEAR_TIE number at most 1 % of the patches of
    every case and every extreme draw -- the condition under which the GPU test leaves them out of its gradient comparison"""
    items = [(table, index, None) for table in (64, 256) for index in range(len(cases.table_of(table)[0]))]
    items += [(64, 0, name) for name in cases.extreme_draws()]
    smallest = np.inf
    for table, index, extreme in items:
        margin = cases.cached_oracle(golden, index, False, np.float64, table=table, extreme=extreme)[3]
        ties = int((margin < cases.NEAR_TIE).sum())
        smallest = min(smallest, margin.min())
        print(f"D = {table} case {index} {extreme or ''}: {ties} near ties of {margin.size} patches, min margin {margin.min():.3g}")
        assert ties <= 0.01 * margin.size, (table, index, extreme)
    print(f"smallest margin {smallest:.3g}")


def test_case_table_exercises_what_it_says():
    """Every shape is safe; case 0 has a duplicate row and a duplicate column position, case 1 non-monotonic positions, case 2
    spans 5 x 2 tiles, case 5 has overlap 0 and all-zero draws, case 6 one patch row"""
    for table in (64, 256):
        rows, patch, _ = cases.table_of(table)
        for shape, stride, _ in rows:
            assert cases.is_safe(shape, patch, stride), (shape, stride)
    pos = [cases.positions(c[0], 8, c[1], cases.case_draws(i)) for i, c in enumerate(cases.CASES)]
    assert len(set(pos[0][0])) < len(pos[0][0]) and len(set(pos[0][1])) < len(pos[0][1])
    assert (np.diff(pos[1][0]) < 0).any() and (np.diff(pos[1][1]) < 0).any()
    ty, tx = cases.TILE
    assert (-(-72 // ty), -(-100 // tx)) == (5, 2)
    assert not any(j.any() for j in cases.case_draws(5)) and len(pos[6][0]) == 1
    text = (REPO / "jolideco_amd" / "csrc" / "gmm_jitter.hip").read_text()
    assert f"GJ_TX = {tx}, GJ_TY = {ty}" in text  # (the tile shape the case table was laid out for)
    extremes = cases.extreme_draws()
    py = cases.positions((40, 44), 8, 4, extremes["alternating"])[0]
    assert (np.diff(py) < 0).any()  # neighbouring rows swap places
    py = cases.positions((40, 44), 8, 4, extremes["coincident"])[0]
    assert (np.diff(py) == 0).any()  # coincident neighbours


# ------------------------------------------------------------------------------------------------ what it switches
def test_constructor_flags_and_refusals():
    import jolideco_amd as jd
    from jolideco_amd.priors import PRIOR_REGISTRY
    from jolideco_amd.priors.patches import MultiScalePrior
    from jolideco_amd.utils.torch import jitter_draws, jitter_grid

    prior = _prior()
    assert prior.jitter is True and prior.cycle_spin_subpix is False and prior.shift_kind == "roll+jitter"
    assert (prior.shardable, prior.supports_fused_step, prior.supports_phases) == (False, False, False)
    assert isinstance(prior, jd.GMMPatchPrior) and jd.JitteredGMMPatchPrior is jd.priors.JitteredGMMPatchPrior
    assert jd.JitteredGMMPatchPrior not in PRIOR_REGISTRY.values() and prior.to_dict()["type"] == "gmm-patches"
    # the three NotImplementedErrors: the plain constructors keep refusing the switch, and the combination with the spin
    with pytest.raises(NotImplementedError, match="jitter .* JitteredGMMPatchPrior"):
        jd.GMMPatchPrior(gmm=_small_gmm(), jitter=True)
    with pytest.raises(NotImplementedError, match="jitter"):
        jd.SubpixelGMMPatchPrior(gmm=_small_gmm(), jitter=True)
    with pytest.raises(NotImplementedError, match="cycle_spin_subpix"):
        jd.JitteredGMMPatchPrior(gmm=_small_gmm(), cycle_spin_subpix=True)
    with pytest.raises(ValueError, match="jitter=True"):
        jd.JitteredGMMPatchPrior(gmm=_small_gmm(), jitter=False)
    assert jd.JitteredGMMPatchPrior(gmm=_small_gmm(), jitter=True).jitter
    # shapes: (37, 41) at stride 4 is not safe, an image without a patch row neither; the message names axis and lengths
    with pytest.raises(ValueError, match="height 37 .* nearest safe height is 36 or 40"):
        prior.check_shape((37, 41))
    with pytest.raises(ValueError, match="width 41 .* nearest safe width is 40 or 44"):
        jitter_grid((40, 41), (8, 8), 4)
    with pytest.raises(ValueError, match="height 12 .* has no jittered patch .* nearest safe height is 16"):
        prior.draw_shifts((12, 40))
    with pytest.raises(ValueError, match="height 37"):
        prior.hessian_ones(torch.ones((1, 1, 37, 40)))
    base_y, base_x = jitter_grid((1, 1, 40, 44), (8, 8), 4)
    assert base_y.tolist() == list(range(4, 32, 4)) and base_x.tolist() == list(range(4, 36, 4))
    for n, safe in ((40, True), (44, True), (72, True), (100, True), (37, False), (41, False), (27, False)):
        assert cases.is_safe((n, n), 8, 4) == safe
    for n, safe in ((48, True), (56, True), (44, False)):
        assert cases.is_safe((n, n), 16, 8) == safe
    jx, jy = jitter_draws(torch.Generator("cpu").manual_seed(3), 5, 3, 2)
    assert jx.shape == (5,) and jy.shape == (3,) and int(jx.abs().max()) <= 2
    # compute_error: the plain prior's conditions; one draw with the flux's shape
    prior.check_hessian_ones()
    state = prior.generator.get_state()
    assert not prior.hessian_ones(torch.ones((1, 1, 40, 44))).any() and not torch.equal(prior.generator.get_state(), state)
    with pytest.raises(NotImplementedError, match="JitteredGMMPatchPrior"):
        MultiScalePrior(prior)
    with pytest.raises(NotImplementedError, match="fused optimizer step"):
        prior.device_fwd_bwd_step(torch.ones((16, 16)), None, 1.0, None)
    with pytest.raises(ValueError, match="pair"):
        prior._split_shifts((1, 2))


def test_strides_below_half_a_patch_are_refused_by_name():
    """No image length is safe below half a patch (safe implies overlap <= stride): the reference's own xfail configuration,
    stride 3 on (37, 37), a 16x16 prior at stride 7 and stride 2 raise a ValueError that says so -- from `jitter_grid`, from
    the constructor (also when the stride is the mixture's ``meta.stride``), from `ops.jitter_counts` -- and never anything
    else; from half a patch on every length either passes or gets a ValueError naming the axis and a safe length."""
    import re

    import jolideco_amd as jd
    from jolideco_amd.ops import jitter_counts
    from jolideco_amd.utils.torch import jitter_grid, jitter_stride_check

    for shape, patch, stride in (((37, 37), 8, 3), ((40, 40), 8, 2), ((64, 64), 16, 7), ((40, 44), 8, 1)):
        for call in (lambda: jitter_grid(shape, (patch, patch), stride), lambda: jitter_counts(shape, patch, stride),
                     lambda: jitter_stride_check(patch, stride)):
            with pytest.raises(ValueError, match=f"stride {stride}: no image height or width is safe .* at least {patch // 2}"):
                call()
    with pytest.raises(ValueError, match="stride 3: no image height or width is safe"):
        _prior(stride=3)
    with pytest.raises(ValueError, match="stride 7: no image height or width is safe"):
        _prior(gmm=_small_gmm(256, 8), stride=7)
    with pytest.raises(ValueError, match="stride 2: no image height or width is safe"):
        jd.JitteredGMMPatchPrior(gmm=_small_gmm(64, 2))  # (the stride of the mixture's meta)
    for stride in (0, 9):
        with pytest.raises(ValueError, match=r"stride in \[1, 8\]"):
            _prior(stride=stride)
    assert _prior(stride=4).stride == 4 and _prior(stride=8).stride == 8 and _prior(gmm=_small_gmm(256, 8), stride=16).stride == 16
    # from half a patch on: every length 1 ... 160 along the height, both patch sizes, every stride
    for patch in (8, 16):
        for stride in range(patch // 2, patch + 1):
            # (one patch column: the smallest safe length; at overlap 0 the arange stops one short of it)
            safe_width = 2 * (patch - stride) + patch + (stride == patch)
            assert not cases.is_safe((safe_width - 1, safe_width), patch, stride)
            assert cases.is_safe((safe_width, safe_width), patch, stride)
            for n in range(1, 161):
                try:
                    base_y, _ = jitter_grid((n, safe_width), (patch, patch), stride)
                    assert cases.is_safe((n, safe_width), patch, stride) and len(base_y) == len(cases.grid((n, safe_width), patch, stride)[0])
                except ValueError as exc:
                    assert not cases.is_safe((n, safe_width), patch, stride)
                    found = re.search(rf"the height {n} .* nearest safe height is (\d+)(?: or (\d+))?$", str(exc))
                    assert found, str(exc)
                    for m in found.groups():
                        assert m is None or (cases.is_safe((int(m), safe_width), patch, stride) and abs(int(m) - n) <= 2 * patch + stride)


def _gmm_library(tmp_path, monkeypatch):
    """A user's GMM library directory with one synthetic model registered as "zoran-weiss" (tests/test_io_formats.py)"""
    from jolideco_amd.priors.patches import GaussianMixtureModel

    arrays = tuple(a.astype(np.float32).astype(np.float64) for a in cpu_ref.synthetic_gmm(3, 64, seed=11, zero_means=False))
    _model(arrays).write(tmp_path / "zw.fits")
    index = {"zoran-weiss": {"filename": "$JOLIDECO_GMM_LIBRARY/zw.fits", "format": "table"}}
    (tmp_path / "jolideco-gmm-library-index.json").write_text(json.dumps(index))
    monkeypatch.setenv("JOLIDECO_GMM_LIBRARY", str(tmp_path))
    return GaussianMixtureModel.from_registry("zoran-weiss")


def test_to_dict_and_from_dict(tmp_path, monkeypatch):
    import jolideco_amd as jd
    from jolideco_amd.priors import Prior

    gmm = _gmm_library(tmp_path, monkeypatch)
    prior = jd.JitteredGMMPatchPrior(gmm=gmm, cycle_spin=False)
    data = prior.to_dict()
    assert data["jitter"] is True and data["cycle_spin_subpix"] is False and data["cycle_spin"] is False
    back = Prior.from_dict(data)
    assert type(back) is jd.JitteredGMMPatchPrior and back.jitter is True and back.cycle_spin is False
    assert back.to_dict() == data
    plain = jd.GMMPatchPrior(gmm=gmm)
    assert plain.to_dict()["jitter"] is False and type(Prior.from_dict(plain.to_dict())) is jd.GMMPatchPrior
    assert type(jd.JitteredGMMPatchPrior.from_dict({k: v for k, v in data.items() if k != "type"})) is jd.JitteredGMMPatchPrior


@pytest.mark.parametrize("format", ["fits", "yaml"])
def test_written_formats_round_trip(format, tmp_path, monkeypatch):
    """The flag travels through the FITS header (PJITTER) and YAML"""
    import jolideco_amd as jd
    from jolideco_amd.utils.io._fitsfile import read_fits

    gmm = _gmm_library(tmp_path, monkeypatch)
    for flag in (True, False):
        component = jd.SpatialFluxComponent(flux_upsampled=torch.ones((1, 1, 16, 16)), prior=(jd.JitteredGMMPatchPrior if flag else jd.GMMPatchPrior)(gmm=gmm))
        filename = tmp_path / f"jitter_{flag}.{format}"
        component.write(filename=filename, format=format)
        back = jd.SpatialFluxComponent.read(filename=filename, format=format)
        assert type(back.prior) is (jd.JitteredGMMPatchPrior if flag else jd.GMMPatchPrior) and back.prior.jitter is flag
        assert back.prior.to_dict() == component.prior.to_dict()
        if format == "fits":
            header = [hdu.header for hdu in read_fits(filename) if "PTYPE" in hdu.header][0]
            assert header["PJITTER"] is flag and header["PSUBSPIN"] is False
        else:
            assert f"jitter: {'true' if flag else 'false'}" in filename.read_text()


# ------------------------------------------------------------------------------------------------ the session
def test_session_flags():
    """A session with such a prior runs by-value epochs only, evaluates the prior whole (no shard, no step in its gather),
    draws with the component's shape and refuses an unsafe component when it is built -- on stand-ins for the session and in
    `FitSession.__init__` up to its refusals (they come before anything touches a device)."""
    import jolideco_amd as jd
    from jolideco_amd.core import FitSession
    from jolideco_amd.distributed import DistContext

    session = FitSession.__new__(FitSession)
    session.has_sparse, session.has_multiscale, session.has_subpix_patches, session.has_jitter_patches = False, False, False, True
    assert session._planned_capable() is False
    assert session._open_policy().startswith("by value") and "JitteredGMMPatchPrior" in session._open_policy()

    class Dist:
        sharded = True

        def shard_range(self, n, shares):
            raise AssertionError("a prior with a jittered patch grid must not be sharded")

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

    jittered = _prior(generator=torch.Generator("cpu").manual_seed(5))
    assert FitSession._prior_rows(Stub(), jittered, State()) is None
    assert not FitSession._fuse_step(One(), State(), jittered)
    session.priors, session.states = [jittered], [State()]
    drawn = session._draw_prior(0)
    want = cases.draw(torch.Generator("cpu").manual_seed(5), (32, 32))
    assert drawn[0] == want[0] and np.array_equal(drawn[1][0].numpy(), want[1][1]) and len(drawn[1][1]) == 5

    datasets = {"o0": {key: np.ones((37, 40), dtype=np.float32) for key in ("counts", "exposure", "background")}}
    datasets["o0"]["psf"] = np.ones((3, 3), dtype=np.float32) / 9
    comps = jd.FluxComponents()
    comps["flux"] = jd.SpatialFluxComponent.from_numpy(flux=np.full((37, 40), 3.0), prior=jittered)
    with pytest.raises(ValueError, match="flux component 'flux': the height 37 .* nearest safe height is 36 or 40"):
        FitSession(jd.MAPDeconvolver(n_epochs=1, device="cuda:0"), datasets, None, comps, DistContext.current())


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_of_the_entry():
    """The new symbol is declared, exported and bound; a null handle, flux, value or jitter array returns JD_ERR_INVALID"""
    from jolideco_amd import _hip

    name = "jd_gmm_prior_jitter_fwd_bwd"
    header = (REPO / "include" / "jolideco_hip.h").read_text()
    assert f"int {name}(jd_gmm* gmm, const float* flux, int H, int W, int stride, int shift_y, int shift_x," in header
    assert "const int* jitter_y_dev, const int* jitter_x_dev, int marginalize, float value_scale," in header
    assert name in (REPO / "jolideco_amd" / "csrc" / "gmm_jitter.hip").read_text()
    assert "gmm_jitter.hip" in (REPO / "jolideco_amd" / "csrc" / "Makefile").read_text()
    lib = _hip.lib()
    assert name in _hip.EXPORTS and hasattr(lib, name) and len(_hip.EXPORTS[name][1]) == 18
    assert lib.jd_gmm_prior_jitter_fwd_bwd(None, None, 40, 44, 4, 0, 0, None, None, 0, 1.0, None, 0, 0.0, None, None, None, None) == -1
    assert b"jd_gmm_prior_jitter_fwd_bwd: null argument" in lib.jd_last_error()


def test_fit_fixture_layout(fixture):
    datasets = unpack_datasets(fixture, "fit/data/")
    assert sorted(datasets) == ["o0", "o1"] and datasets["o0"]["counts"].shape == cases.FIT_SHAPE
    assert fixture["fit/flux_init"].shape == fixture["fit/flux_final"].shape == cases.FIT_SHAPE
    assert len(fixture["fit/trace/total"]) == cases.FIT_EPOCHS

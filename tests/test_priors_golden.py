"""CPU: the priors of a point-source layer -- `cycle_spin_subpix=True` of InverseGammaPrior / ExponentialPrior and
SmoothnessPrior -- against tests/golden/priors.npz (generated from the live reference by tools/make_golden_priors.py): the
oracles of tests/prior_cases.py, the host logic (draws, kernel array, dict / FITS / YAML round trips, slot planning) and the
argument checks of the two C entries.  Nothing here needs a GPU."""
import types

import numpy as np
import pytest
import torch

import prior_cases as cases


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("priors")


@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_sparse_oracle_matches_the_reference(fixture, kind):
    x0, y0 = fixture[f"{kind}/offsets"]
    value, grad = cases.sparse_oracle(fixture["flux"], kind, x0, y0, dtype=np.float32)
    assert value == float(fixture[f"{kind}/value"])
    assert np.array_equal(grad.astype(np.float32), fixture[f"{kind}/grad"])
    value64, grad64 = cases.sparse_oracle(fixture["flux"], kind, x0, y0, dtype=np.float64)
    assert abs(value64 - value) <= 1e-5 * abs(value64) and cases.rel_linf(grad, grad64) < 1e-5


@pytest.mark.parametrize("width", cases.SMOOTH_WIDTHS)
def test_smoothness_oracle_and_kernel_match_the_reference(fixture, width):
    from jolideco_amd.priors import SmoothnessPrior
    from jolideco_amd.utils.numpy import gaussian_kernel_2d

    stored = fixture[f"smooth/{width}/kernel"]
    assert stored.shape[0] % 2 == 1 and stored.shape[0] >= 8 * width and stored.shape[0] == (17 if width == 2 else 13)
    for array in (gaussian_kernel_2d(width), SmoothnessPrior(width=width).kernel_numpy, cases.gaussian_kernel(width)):
        assert array.dtype == np.float64 and array.shape == stored.shape
        assert np.max(np.abs(array - stored)) <= 1e-15
    assert abs(stored.sum() - 1.0) < 1e-14 and np.array_equal(stored, stored.T) and np.array_equal(stored, stored[::-1, ::-1])
    flux = torch.from_numpy(fixture["flux"][None, None]).requires_grad_(True)
    value = cases.SmoothnessPriorRef(width)(flux)
    value.backward()
    assert float(value.detach()) == float(fixture[f"smooth/{width}/value"])
    assert np.array_equal(flux.grad.numpy()[0, 0], fixture[f"smooth/{width}/grad"])
    value64, grad64 = cases.smoothness_oracle(fixture["flux"], stored, np.float64)
    assert abs(value64 - float(value.detach())) <= 1e-6 * abs(value64)
    assert cases.rel_linf(fixture[f"smooth/{width}/grad"], grad64) < 1e-6


def test_constructors_and_dicts():
    import jolideco_amd as jd
    from jolideco_amd.priors import PRIOR_REGISTRY, Prior, SmoothnessPrior

    assert jd.SmoothnessPrior is SmoothnessPrior and PRIOR_REGISTRY["smooth"] is SmoothnessPrior
    for cls, extra in ((jd.InverseGammaPrior, {"alpha": 10.0, "beta": 1.5}), (jd.ExponentialPrior, {"alpha": 10.0})):
        prior = cls(cycle_spin_subpix=True)
        assert prior.cycle_spin_subpix is True and prior.draws_shifts
        assert prior.generator.device.type == "cpu" and prior.generator.initial_seed() == torch.Generator("cpu").initial_seed()
        data = prior.to_dict()
        assert data == dict({"type": data["type"], "cycle_spin_subpix": True}, **extra)
        back = Prior.from_dict(data)
        assert type(back) is cls and back.cycle_spin_subpix is True and back.to_dict() == data
        plain = cls()
        assert plain.cycle_spin_subpix is False and not plain.draws_shifts and plain.to_dict()["cycle_spin_subpix"] is False
    smooth = Prior.from_dict({"type": "smooth"})
    assert isinstance(smooth, SmoothnessPrior) and smooth.to_dict() == {"type": "smooth", "width": 2.0}
    narrow = Prior.from_dict({"type": "smooth", "width": 1.5})
    assert narrow.to_dict() == {"type": "smooth", "width": 1.5} and narrow.kernel.shape == (1, 1, 13, 13)
    assert narrow.kernel.dtype == torch.float64
    with pytest.raises(ValueError):
        SmoothnessPrior(width=0)


@pytest.mark.parametrize("format", ["fits", "yaml"])
def test_written_formats_round_trip(format, tmp_path):
    """The option and the smoothness prior travel through the FITS header (PSUBSPIN, PWIDTH) and YAML."""
    import jolideco_amd as jd
    from jolideco_amd.utils.io._fitsfile import read_fits

    for name, prior in (("points", jd.InverseGammaPrior(alpha=4, beta=2.5, cycle_spin_subpix=True)),
                        ("expo", jd.ExponentialPrior(alpha=3, cycle_spin_subpix=True)),
                        ("smooth", jd.SmoothnessPrior(width=1.5))):
        component = jd.SpatialFluxComponent(flux_upsampled=torch.ones((1, 1, 16, 16)), prior=prior)
        filename = tmp_path / f"{name}.{format}"
        component.write(filename=filename, format=format)
        back = jd.SpatialFluxComponent.read(filename=filename, format=format)
        assert type(back.prior) is type(prior) and back.prior.to_dict() == prior.to_dict()
        if format == "fits":
            header = [hdu.header for hdu in read_fits(filename) if "PTYPE" in hdu.header][0]
            if name == "smooth":
                assert header["PTYPE"] == "smooth" and header["PWIDTH"] == 1.5
            else:
                assert header["PSUBSPIN"] is True
        else:
            text = filename.read_text()
            assert ("width: 1.5" in text) if name == "smooth" else ("cycle_spin_subpix: true" in text)


def test_draw_order_and_numbers(fixture):
    """x first, then y, float32 `rand(1) - 0.5`: the fixture's offsets from the fixture's seed; `last_shifts` follows."""
    import jolideco_amd as jd

    generator = torch.Generator("cpu").manual_seed(cases.FIXTURE_SEED)
    prior = jd.InverseGammaPrior(cycle_spin_subpix=True, generator=generator)
    drawn = prior.draw_shifts()
    assert isinstance(drawn[0], float) and isinstance(drawn[1], float)
    assert drawn == tuple(fixture["inverse-gamma/offsets"]) == tuple(fixture["exponential/offsets"]) == prior.last_shifts
    replay = torch.Generator("cpu").manual_seed(cases.FIXTURE_SEED)
    x0 = torch.rand(1, generator=replay) - 0.5
    y0 = torch.rand(1, generator=replay) - 0.5
    assert drawn == (float(x0), float(y0)) and x0.dtype == torch.float32
    assert np.float32(drawn[0]) == drawn[0] and np.float32(drawn[1]) == drawn[1]  # exact images of float32 numbers
    # default generators: the reference's default seed, so a default-constructed fit draws the reference's numbers
    ours, theirs = jd.ExponentialPrior(cycle_spin_subpix=True), cases.SubpixPriorRef("exponential")
    assert [ours.draw_shifts() for _ in range(5)] == [cases.draw_offsets(theirs.generator) for _ in range(5)]


def test_batched_draws_equal_single_draws():
    """`draw_shifts_many(n)` may take its numbers from one `rand(2 n)` call only because torch's CPU generator hands out the
    same float32 numbers as 2 n single draws and ends in the same state -- checked for 1 .. 39 pairs and sizes around the
    batch limit."""
    from jolideco_amd.priors import InverseGammaPrior
    from jolideco_amd.utils.torch import SUBPIX_BATCH_MAX, subpixel_offsets, subpixel_offsets_many

    for n in list(range(1, 40)) + [64, 100, 255, 256, 257, SUBPIX_BATCH_MAX // 2, SUBPIX_BATCH_MAX // 2 + 1]:
        a, b = torch.Generator("cpu").manual_seed(5 + n), torch.Generator("cpu").manual_seed(5 + n)
        batch = torch.rand(2 * n, generator=a)
        single = torch.cat([torch.rand(1, generator=b) for _ in range(2 * n)])
        assert torch.equal(batch, single) and torch.equal(a.get_state(), b.get_state()), n
        a, b = torch.Generator("cpu").manual_seed(9 + n), torch.Generator("cpu").manual_seed(9 + n)
        assert subpixel_offsets_many(a, n) == [subpixel_offsets(b) for _ in range(n)], n
        assert torch.equal(a.get_state(), b.get_state()), n
    prior = InverseGammaPrior(cycle_spin_subpix=True, generator=torch.Generator("cpu").manual_seed(3))
    twin = InverseGammaPrior(cycle_spin_subpix=True, generator=torch.Generator("cpu").manual_seed(3))
    many = prior.draw_shifts_many(3)
    assert many == [twin.draw_shifts() for _ in range(3)] and prior.last_shifts == many[-1]
    assert prior.draw_shifts() == twin.draw_shifts()


def test_generator_must_live_on_the_host():
    import jolideco_amd as jd

    device_generator = types.SimpleNamespace(device=torch.device("cuda"))
    for cls in (jd.InverseGammaPrior, jd.ExponentialPrior):
        with pytest.raises(ValueError, match="CPU generator"):
            cls(cycle_spin_subpix=True, generator=device_generator)


def test_hessian_ones_with_the_option_matches_autograd():
    """Kt (v''(s) * K 1) / n against torch's double backward of the same log-prior, same draw."""
    from jolideco_amd.priors import InverseGammaPrior

    flux = torch.tensor(np.random.RandomState(3).gamma(2.0, size=(1, 1, 6, 7)).astype(np.float32) + 0.2)
    prior = InverseGammaPrior(alpha=0.1, cycle_spin_subpix=True, generator=torch.Generator("cpu").manual_seed(8))
    offsets = cases.draw_offsets(torch.Generator("cpu").manual_seed(8))

    def log_prior(x):
        return cases.sparse_log_prior(x, "inverse-gamma", 0.1, 1.5, cases.subpix_kernel(*offsets), 0.0)

    expected = torch.autograd.functional.vhp(log_prior, flux, v=torch.ones_like(flux))[1]
    got = prior.hessian_ones(flux)
    assert prior.last_shifts == offsets
    np.testing.assert_allclose(got.numpy(), expected.numpy(), rtol=2e-5, atol=1e-8)


def test_cabi_refusals():
    """The new entries return JD_ERR_INVALID (-1) with a message before they touch a device."""
    from jolideco_amd import _hip

    if not _hip.library_path().exists():
        import __graft_entry__

        __graft_entry__.build()
    lib = _hip.lib()
    assert {"jd_elementwise_prior_subpix_fwd_bwd", "jd_smoothness_prior_fwd_bwd"} <= set(_hip.EXPORTS)
    fn = lib.jd_elementwise_prior_subpix_fwd_bwd
    fake = 4096  # a non-null pointer: every call below must return before reading it
    assert fn(7, fake, 8, 8, 10.0, 1.5, 0.0, 0.0, 0.0, None, fake, 0.0, None, None) == -1
    assert b"kind must be 1" in lib.jd_last_error()
    assert fn(1, None, 8, 8, 10.0, 1.5, 0.0, 0.0, 0.0, None, fake, 0.0, None, None) == -1
    assert fn(1, fake, 8, 8, 10.0, 1.5, 0.0, 0.0, 0.0, None, None, 0.0, None, None) == -1
    assert b"null argument" in lib.jd_last_error()
    assert fn(2, fake, 0, 8, 10.0, 0.0, 0.0, 0.0, 0.0, None, fake, 0.0, None, None) == -1
    assert fn(2, fake, 8, -1, 10.0, 0.0, 0.0, 0.0, 0.0, None, fake, 0.0, None, None) == -1
    for x0, y0 in ((0.6, 0.0), (0.0, -0.50001), (float("nan"), 0.0), (0.0, float("inf"))):
        assert fn(1, fake, 8, 8, 10.0, 1.5, 0.0, x0, y0, None, fake, 0.0, None, None) == -1
        assert b"not in [-0.5, 0.5]" in lib.jd_last_error()
    assert lib.jd_smoothness_prior_fwd_bwd(None, fake, fake, fake, 0.0, None, None) == -1
    assert b"null argument" in lib.jd_last_error()
    assert lib.jd_kernel_name(_hip.KERNEL_IDS["elementwise_subpix"]) == b"elementwise_prior_subpix_kernel"
    assert lib.jd_kernel_name(_hip.KERNEL_IDS["smoothness"]) == b"smoothness_prior_kernel"
    assert _hip.KERNEL_IDS["elementwise_subpix"] == _hip.KERNEL_IDS["poisson_mixed"] + 1


def _session_standin(priors, n_local, joint):
    from jolideco_amd.core import FitSession

    session = FitSession.__new__(FitSession)
    session.priors, session.joint = priors, joint
    session.local_idx = [(i, i) for i in range(n_local)]
    session.cal_optimizers = [None] * n_local
    return session


@pytest.mark.parametrize("joint", [False, True])
def test_sessions_without_the_option_plan_the_same_slots(joint):
    """Only priors that draw get a slot: a session whose sparse priors have the option off plans what it planned before
    they could draw at all (one slot per evaluation of the cycle-spin prior); with the option on, one more per evaluation."""
    import jolideco_amd as jd

    class Rolls:  # stand-in for the GMM prior: draws integer rolls
        def draw_shifts(self):
            return (0, 0)

    n_local = 3
    n_eval = 1 if joint else n_local + 1
    plain = [Rolls(), jd.InverseGammaPrior(), jd.ExponentialPrior(), jd.UniformPrior(), jd.SmoothnessPrior()]
    drawing, n_shift, n_flux, cal_groups, n_cal = _session_standin(plain, n_local, joint)._plan_slots()
    before = [ci for ci, prior in enumerate(plain) if isinstance(prior, Rolls)]  # what had `draw_shifts` before
    assert drawing == before == [0] and n_shift == n_eval and n_cal == 0 and n_flux == (1 if joint else n_local)
    spun = [Rolls(), jd.InverseGammaPrior(cycle_spin_subpix=True), jd.ExponentialPrior(), jd.ExponentialPrior(cycle_spin_subpix=True)]
    drawing, n_shift, _, _, _ = _session_standin(spun, n_local, joint)._plan_slots()
    assert drawing == [0, 1, 3] and n_shift == 3 * n_eval

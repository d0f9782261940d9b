"""CPU: the options of torch.optim.Adam / SGD in `MAPDeconvolver(optimizer_kwargs=...)` -- what constructs, what raises
as torch raises, what stays refused; what an active option switches off in a session; the argument checks of
jd_optimizer_step / jd_optimizer_step_multi; and the oracle of tests/optimizer_option_cases.py: finite in float32 on
every case of tests/test_gpu_optimizer_options.py, and the two details of torch.optim a kernel can get wrong."""
import ctypes
import types

import numpy as np
import pytest
import torch

import optimizer_option_cases as cases

ADAM_SETS = [name for name, (sgd, _) in cases.OPTION_SETS.items() if not sgd]
SGD_SETS = [name for name, (sgd, _) in cases.OPTION_SETS.items() if sgd]


def deconvolver(optimizer_type="adam", **kwargs):
    from jolideco_amd import MAPDeconvolver

    return MAPDeconvolver(n_epochs=1, display_progress=False, device="cuda", optimizer_type=optimizer_type,
                          optimizer_kwargs=kwargs or None)


# ------------------------------------------------------------------------------------------------------------ constructor
def test_weight_decay_constructs():
    from jolideco_amd.core import optimizer_options

    cfg = deconvolver(weight_decay=1e-3)
    assert optimizer_options(cfg) == ({"weight_decay": 1e-3, "amsgrad": False, "decoupled_weight_decay": False}, True)


@pytest.mark.parametrize("name", sorted(cases.OPTION_SETS))
def test_every_option_set_constructs_and_is_active(name):
    from jolideco_amd.core import optimizer_options

    sgd, options = cases.OPTION_SETS[name]
    cfg = deconvolver("sgd" if sgd else "adam", **options)
    got, active = optimizer_options(cfg)
    assert active and all(got[key] == value for key, value in options.items())
    assert "optimizer_kwargs" not in cfg.to_dict() and set(cfg.to_dict()) == set(deconvolver().to_dict())


@pytest.mark.parametrize("optimizer_type", ["adam", "sgd"])
def test_options_at_their_defaults_are_not_active(optimizer_type):
    from jolideco_amd.core import OPTIMIZER_OPTIONS, optimizer_options

    defaults = OPTIMIZER_OPTIONS[optimizer_type]
    assert not optimizer_options(deconvolver(optimizer_type))[1]
    assert not optimizer_options(deconvolver(optimizer_type, **defaults))[1]
    # (the defaults are torch's: its optimizer stores exactly these)
    optimizer = (torch.optim.Adam if optimizer_type == "adam" else torch.optim.SGD)([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    assert {key: optimizer.defaults[key] for key in defaults} == defaults


@pytest.mark.parametrize("optimizer_type,kwargs,message", [
    ("adam", {"weight_decay": -1e-3}, "Invalid weight_decay value"),
    ("sgd", {"weight_decay": -1e-3}, "Invalid weight_decay value"),
    ("sgd", {"momentum": -0.5}, "Invalid momentum value"),
    ("sgd", {"nesterov": True}, "Nesterov momentum requires a momentum and zero dampening"),
    ("sgd", {"nesterov": True, "momentum": 0.9, "dampening": 0.1}, "Nesterov momentum requires a momentum and zero dampening"),
])
def test_invalid_values_raise_the_value_errors_of_torch(optimizer_type, kwargs, message):
    with pytest.raises(ValueError, match=message):
        deconvolver(optimizer_type, **kwargs)
    optimizer = torch.optim.Adam if optimizer_type == "adam" else torch.optim.SGD
    with pytest.raises(ValueError, match=message):  # (torch says the same)
        optimizer([torch.nn.Parameter(torch.zeros(1))], lr=0.1, **kwargs)


@pytest.mark.parametrize("optimizer_type", ["adam", "sgd"])
@pytest.mark.parametrize("key", ["maximize", "foreach", "fused", "capturable", "differentiable"])
def test_refused_options_stay_refused(optimizer_type, key):
    with pytest.raises(NotImplementedError, match=key):
        deconvolver(optimizer_type, **{key: True})


def test_an_option_of_the_other_optimizer_is_refused():
    with pytest.raises(NotImplementedError, match="momentum"):
        deconvolver("adam", momentum=0.9)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        deconvolver("sgd", amsgrad=True)


# ---------------------------------------------------------------------------------------------------------------- session
def session_standin(cfg):
    from jolideco_amd.core import FitSession

    session = FitSession.__new__(FitSession)
    session.cfg, session.fuse_optimizer_step = cfg, True
    session.dist = types.SimpleNamespace(sharded=False, world_size=1)
    session.has_sparse, session.has_multiscale, session._planned_ok, session.comm_events, session.n_val = False, False, True, None, 0
    image = lambda: torch.zeros(8, 16)  # noqa: E731
    state = types.SimpleNamespace(frozen=False, theta=image(), flux=[image(), image()], grad=image(), exp_avg=image(),
                                  exp_avg_sq=image(), mask=None)
    prior = types.SimpleNamespace(supports_fused_step=True, stride=4)
    return session, state, prior


CONFIGS = [("adam", {}, False), ("sgd", {}, False), ("adam", {"weight_decay": 0, "amsgrad": False}, False),
           ("sgd", {"momentum": 0, "nesterov": False}, False)]
CONFIGS += [("sgd" if sgd else "adam", options, True) for sgd, options in cases.OPTION_SETS.values()]


@pytest.mark.parametrize("optimizer_type,kwargs,active", CONFIGS)
def test_an_active_option_takes_the_step_out_of_the_fused_kernels_and_a_momentum_out_of_planned_epochs(optimizer_type, kwargs, active):
    session, state, prior = session_standin(deconvolver(optimizer_type, **kwargs))
    assert bool(session._fuse_step(state, prior)) == (not active)
    assert bool(session._fuse_band_step(state)) == (not active)
    assert session._planned_capable() == (not kwargs.get("momentum"))


def test_steppers_allocate_the_state_of_the_options_when_they_are_built():
    from jolideco_amd.core import _CalibrationStepper

    params = [torch.nn.Parameter(torch.zeros(1, 2)), torch.nn.Parameter(torch.zeros(1))]
    plain = _CalibrationStepper(params, deconvolver())
    assert all(sorted(state) == ["exp_avg", "exp_avg_sq", "step"] for state in plain.state)
    amsgrad = _CalibrationStepper(params, deconvolver(amsgrad=True))
    assert all(state["max_exp_avg_sq"].shape == p.shape for p, state in zip(params, amsgrad.state))
    momentum = _CalibrationStepper(params, deconvolver("sgd", momentum=0.9))
    assert all(state["momentum_buffer"].shape == p.shape and state["first_step"] is True for p, state in zip(params, momentum.state))


# ------------------------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def lib():
    from jolideco_amd import _hip

    if not _hip.library_path().exists():
        import __graft_entry__

        __graft_entry__.build()
    return _hip.lib()


FAKE = 4096  # a non-null pointer: every call below must return before reading it


def options_struct(**fields):
    from jolideco_amd import _hip

    base = dict(kind=_hip.OPTIMIZER_ADAM, step_size=0.1, beta1=0.9, beta2=0.999, one_minus_beta1=0.1, one_minus_beta2=0.001,
                bias2_sqrt=1.0, eps=1e-8, lr=0.1)
    return _hip.OptimizerOptions(**{**base, **fields})


INVALID_OPTIONS = [
    (dict(kind=7), b"unknown optimizer kind"),
    (dict(weight_decay=-1.0), b"must be finite and >= 0"),
    (dict(lr=float("nan")), b"must be finite and >= 0"),
    (dict(kind=1, momentum=-0.1), b"must be finite and >= 0"),
    (dict(kind=1, dampening=float("inf")), b"must be finite and >= 0"),
    (dict(kind=1, nesterov=1), b"nesterov needs a momentum and zero dampening"),
    (dict(kind=1, nesterov=1, momentum=0.9, dampening=0.1), b"nesterov needs a momentum and zero dampening"),
    (dict(kind=0, momentum=0.9), b"options of SGD"),
    (dict(kind=0, nesterov=1), b"options of SGD"),
    (dict(kind=1, amsgrad=1), b"options of Adam"),
    (dict(kind=1, decoupled_weight_decay=1), b"options of Adam"),
]


def test_the_entries_are_exported():
    from jolideco_amd import _hip

    assert {"jd_optimizer_step", "jd_optimizer_step_multi"} <= set(_hip.EXPORTS)
    assert ctypes.sizeof(_hip.OptimizerOptions) == 80  # (int + 7 floats | 4 doubles | 4 ints: no padding)


def test_optimizer_step_checks_its_arguments(lib):
    def call(theta=FAKE, flux_in=FAKE, flux_out=FAKE, grad=FAKE, m=FAKE, v=FAKE, vmax=None, buf=None, n=16, options=None,
             no_options=False, **fields):
        options = None if no_options else ctypes.byref(options_struct(**fields))
        return lib.jd_optimizer_step(theta, flux_in, flux_out, grad, m, v, vmax, buf, None, n, options, 0, 1, None, None)

    for missing in ("theta", "flux_in", "flux_out", "grad"):
        assert call(**{missing: None}, weight_decay=0.1) == -1 and b"null argument or n == 0" in lib.jd_last_error()
    assert call(n=0, weight_decay=0.1) == -1 and b"null argument or n == 0" in lib.jd_last_error()
    assert call(no_options=True) == -1 and b"null options" in lib.jd_last_error()
    assert call(m=None, weight_decay=0.1) == -1 and b"Adam needs its moment images" in lib.jd_last_error()
    assert call(v=None, weight_decay=0.1) == -1 and b"Adam needs its moment images" in lib.jd_last_error()
    assert call(amsgrad=1) == -1 and b"amsgrad needs max_exp_avg_sq" in lib.jd_last_error()
    assert call(buf=FAKE, amsgrad=1) == -1 and b"amsgrad needs max_exp_avg_sq" in lib.jd_last_error()
    assert call(m=None, v=None, kind=1, momentum=0.9) == -1 and b"momentum needs momentum_buffer" in lib.jd_last_error()
    assert call(vmax=FAKE, kind=1, momentum=0.9) == -1 and b"momentum needs momentum_buffer" in lib.jd_last_error()
    for fields, message in INVALID_OPTIONS:
        assert call(vmax=FAKE, buf=FAKE, **fields) == -1, fields
        assert message in lib.jd_last_error(), (fields, lib.jd_last_error())


def test_optimizer_step_multi_checks_its_arguments(lib):
    def pointers(n, value=FAKE):
        return (ctypes.c_void_p * n)(*([value] * n))

    def call(n=3, theta="fake", grad="fake", m="fake", v="fake", vmax=None, buf=None, sizes="fake", terms=True, first=None,
             no_options=False, **fields):
        length = max(n, 1)
        fill = lambda a: pointers(length) if isinstance(a, str) else a  # noqa: E731
        sizes = (ctypes.c_int * length)(*([2] * length)) if isinstance(sizes, str) else sizes
        floats = (ctypes.c_float * length)(*([1.0] * length)) if terms else None
        options = None if no_options else ctypes.byref(options_struct(**fields))
        return lib.jd_optimizer_step_multi(n, fill(theta), fill(grad), fill(m), fill(v), fill(vmax), fill(buf), sizes, floats, floats,
                                           first, options, None, None)

    for n in (0, -1, 65):
        assert call(n=n, weight_decay=0.1) == -1 and b"not in [1, 64]" in lib.jd_last_error()
    for missing in ("theta", "grad", "sizes"):
        assert call(**{missing: None}, weight_decay=0.1) == -1 and b"null argument" in lib.jd_last_error()
    assert call(no_options=True) == -1 and b"null options" in lib.jd_last_error()
    assert call(m=None, weight_decay=0.1) == -1 and b"Adam needs its moments and bias terms" in lib.jd_last_error()
    assert call(terms=False, weight_decay=0.1) == -1 and b"Adam needs its moments and bias terms" in lib.jd_last_error()
    assert call(amsgrad=1) == -1 and b"amsgrad needs max_exp_avg_sq" in lib.jd_last_error()
    first = (ctypes.c_int * 3)(1, 0, 1)
    assert call(kind=1, momentum=0.9, first=first) == -1 and b"momentum needs momentum_buffer" in lib.jd_last_error()
    assert call(kind=1, momentum=0.9, buf="fake") == -1 and b"momentum needs momentum_buffer and first_step" in lib.jd_last_error()
    holes = pointers(3)
    holes[1] = None
    assert call(theta=holes, weight_decay=0.1) == -1 and b"null tensor 1" in lib.jd_last_error()
    assert call(vmax=holes, amsgrad=1) == -1 and b"null tensor 1" in lib.jd_last_error()
    assert call(buf=holes, kind=1, momentum=0.9, first=first) == -1 and b"null tensor 1" in lib.jd_last_error()
    assert call(sizes=(ctypes.c_int * 3)(2, 2, 0), weight_decay=0.1) == -1 and b"null tensor 2" in lib.jd_last_error()
    for fields, message in INVALID_OPTIONS:
        assert call(vmax="fake", buf="fake", first=first, **fields) == -1, fields
        assert message in lib.jd_last_error(), (fields, lib.jd_last_error())


# ----------------------------------------------------------------------------------------------------------------- oracle
SIZES = (4, 1020, 1021)


@pytest.mark.parametrize("name", sorted(cases.OPTION_SETS))
def test_float32_oracle_stays_finite_on_every_case(name):
    """Every (size, flux form, mask) of the GPU module's step test: the float32 oracle ends finite, so its error against
    float64 is a figure a bound can be taken from; theta moves in both."""
    worst = {}
    for n in SIZES + ((3072,) if name in ("adam-wd-amsgrad", "sgd-momentum-wd-nesterov") else ()):
        for linear in (False, True):
            for masked in (False, True):
                tr = cases.trajectory(name, n, masked, linear)
                for ref in ("ref64", "ref32"):
                    for key, arrays in tr[ref].items():
                        assert len(arrays) == cases.N_STEPS and all(np.isfinite(a).all() for a in arrays), (n, linear, masked, ref, key)
                assert not np.array_equal(tr["ref32"]["theta"][-1], tr["theta0"])
                for step in range(cases.N_STEPS):
                    for key, value in cases.errors(tr["ref32"], tr["ref64"], tr["mask"], step).items():
                        worst[key] = max(worst.get(key, 0.0), value)
    print(f"\nfloat32 oracle {name}: " + ", ".join(f"{key} {value:.2e}" for key, value in worst.items()))
    sgd, options = cases.OPTION_SETS[name]
    expected = {"theta", "flux"} | ({"momentum_buffer"} if options.get("momentum") else set())
    if not sgd:
        expected |= {"exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if options.get("amsgrad") else set())
    assert set(worst) == expected


@pytest.mark.parametrize("name", sorted(cases.OPTION_SETS))
def test_the_options_reach_the_oracle(name):
    """The same run without the kwargs ends elsewhere: an option dropped on the way to torch.optim would pass every bound."""
    tr = cases.trajectory(name, 1021, True, False)
    bare = cases.oracle(tr["theta0"], tr["mask"], tr["grads"], linear=False, sgd=tr["sgd"], lr=tr["lr"], options={},
                        state0={k: v for k, v in tr["state0"].items() if k != "max_exp_avg_sq"} or None, step0=tr["step0"])
    assert not np.array_equal(bare["theta"][-1], tr["ref64"]["theta"][-1])


@pytest.mark.parametrize("name", [n for n, (_, o) in cases.OPTION_SETS.items() if o.get("weight_decay")])
@pytest.mark.parametrize("linear", [False, True], ids=["log", "linear"])
def test_weight_decay_moves_theta_under_the_mask_and_the_flux_stays_zero(name, linear):
    tr = cases.trajectory(name, 1021, True, linear)
    off = tr["mask"] == 0
    for ref in ("ref64", "ref32"):
        assert np.all(tr[ref]["theta"][-1][off] != tr["theta0"][off])
        assert all(np.all(flux[off] == 0) for flux in tr[ref]["flux"])


@pytest.mark.parametrize("name", [n for n, (_, o) in cases.OPTION_SETS.items() if not o.get("weight_decay")])
def test_without_weight_decay_a_masked_theta_keeps_its_bits(name):
    tr = cases.trajectory(name, 1021, True, False)
    off = tr["mask"] == 0
    assert all(np.array_equal(theta[off], tr["theta0"][off]) for theta in tr["ref32"]["theta"])


def test_the_first_momentum_step_takes_the_gradient_undamped():
    """After step 1 the buffer is the gradient of that step, weight decay included, whatever the dampening; step 2 damps."""
    n = 1021
    tr = cases.trajectory("sgd-momentum-dampening", n, False, True)
    first, second = tr["ref64"]["momentum_buffer"][:2]
    g0, g1 = tr["grads"][0].astype(np.float64), tr["grads"][1].astype(np.float64)
    assert np.array_equal(first, g0)  # (linear, no mask: d flux / d theta = 1)
    np.testing.assert_allclose(second, 0.9 * g0 + 0.75 * g1, rtol=1e-12, atol=1e-300)

"""`FitSession._enqueue_epoch` is the one place that spells out an epoch.  On recording stand-ins (epoch_sequence_cases.py: no
library, CPU tensors) it must make, call for call, the calls that the two bodies it replaced made: likelihood and prior calls
with their buffers, `accumulate` flags, coefficients, shifts, phases and patch rows, the collectives and their names, the
optimizer steps with their numbers and `stepped` sets (and the `last_shifts` a replaced step would read), the calibration
steps, the draws from every generator.  The logs
under tests/golden/ were recorded from the by-value body of the commit before (tools/make_golden_epoch_sequences.py), less
the fill launch of a uniform prior -- the one launch the single body drops."""
import json
from pathlib import Path

import pytest

import epoch_sequence_cases as cases
from jolideco_amd import core

GOLDEN = json.loads((Path(__file__).parent / "golden" / "epoch_sequences.json").read_text())


def test_every_case_has_a_recorded_log():
    assert sorted(GOLDEN["cases"]) == sorted(cases.CASES) and GOLDEN["n_epochs"] == cases.N_EPOCHS
    # Where both bodies of the commit before applied they made the same calls, with one difference that no call shows: its
    # `_plan_by_value` drew the shifts of a whole sequential epoch up front, so DURING a step `last_shifts` of a prior was the
    # trace's draw, not the step's (a replaced `_optimizer_step` that records the gradient reads it: conftest.py's
    # `run_recording_steps`).  The by-value body's behaviour is the one kept and recorded.
    for case, found in GOLDEN["disagreements"].items():
        assert case.startswith("sequential-")
        (old,), (new,) = found["by_value"], found["planned"]
        assert old["kind"] == "optimizer-step" and {k for k in old if old[k] != new[k]} == {"last_shifts"}


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_the_epoch_body_makes_the_recorded_calls(case):
    log = cases.run_case(core, case, lambda session: session._enqueue_epoch(session._plan_by_value()))
    log = json.loads(json.dumps(log))
    expected = GOLDEN["cases"][case]
    for i, (got, want) in enumerate(zip(log, expected)):
        assert got == want, f"call {i} of {case}"
    assert len(log) == len(expected)
    assert not any(entry["kind"] == "uniform-fill" for entry in log)


def test_a_planned_parameter_that_lost_its_gradient_raises():
    """The plan of an epoch gives every calibration parameter that had a gradient after the epoch before a device slot for
    its bias terms: one without a gradient now must raise (before any launch), through the one step function and through a
    stepper, and its count stays."""
    import torch

    cfg = core.MAPDeconvolver(device="cuda", display_progress=False)
    stepper = core._CalibrationStepper([torch.nn.Parameter(torch.zeros(2))], cfg)
    items = list(zip(stepper.params, stepper.state))
    assert items[0][0].grad is None
    bias_dev = torch.zeros(2)
    with pytest.raises(RuntimeError, match="lost its gradient"):
        core._step_parameters(cfg, items, {}, bias_dev)
    with pytest.raises(RuntimeError, match="lost its gradient"):
        stepper.step(bias_dev)
    assert stepper.state[0]["step"] == 0

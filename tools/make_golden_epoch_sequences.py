"""Write tests/golden/epoch_sequences.json: the ordered calls that the epoch body of ANOTHER checkout of this project makes on
the recording stand-ins of tests/epoch_sequence_cases.py (three epochs per case).

    python tools/make_golden_epoch_sequences.py /path/to/checkout

The checkout is one that still has `FitSession._epoch_by_value` (the commit before the two epoch bodies became one): every
case is run through it, and -- where it applies: one process, no validation datasets -- through
`_enqueue_epoch(_plan_by_value())` as well.  The by-value body's log is what is written, less the fill launches of a uniform
prior (the one launch the single body was allowed to drop).  Where the checkout's two bodies disagree beyond that, the case
and the first differing entry are printed and written under "disagreements"."""
import importlib
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def main(checkout):
    sys.path.insert(0, str(Path(checkout).resolve()))
    sys.path.insert(1, str(REPO / "tests"))
    core = importlib.import_module("jolideco_amd.core")
    assert Path(core.__file__).resolve().is_relative_to(Path(checkout).resolve()), core.__file__
    import epoch_sequence_cases as cases

    def by_value(session):
        session._epoch_by_value()

    def planned_by_value(session):
        session._enqueue_epoch(session._plan_by_value())

    def kept(log):
        return json.loads(json.dumps([entry for entry in log if entry["kind"] != "uniform-fill"]))

    golden, disagreements = {}, {}
    for name, case in cases.CASES.items():
        golden[name] = kept(cases.run_case(core, name, by_value))
        opt = dict(cases.DEFAULTS, **case)
        if opt["world"] is None and not opt["n_val"]:
            other = kept(cases.run_case(core, name, planned_by_value))
            if other != golden[name]:
                first = next((i for i, (a, b) in enumerate(zip(golden[name], other)) if a != b), min(len(other), len(golden[name])))
                disagreements[name] = {"entry": first, "by_value": golden[name][first : first + 1], "planned": other[first : first + 1]}
                print(f"{name}: the two bodies disagree at entry {first}: {disagreements[name]}")
        print(f"{name}: {len(golden[name])} calls")
    out = REPO / "tests" / "golden" / "epoch_sequences.json"
    # (one call per line: a changed call shows as one changed line)
    lines = [f'{{"n_epochs": {cases.N_EPOCHS}, "disagreements": {json.dumps(disagreements)}, "cases": {{']
    for k, (name, log) in enumerate(golden.items()):
        lines.append(f"{json.dumps(name)}: [")
        lines += [json.dumps(entry, separators=(",", ":")) + ("," if i + 1 < len(log) else "") for i, entry in enumerate(log)]
        lines.append("]" + ("," if k + 1 < len(golden) else ""))
    out.write_text("\n".join(lines + ["}}"]) + "\n")
    print(f"wrote {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])

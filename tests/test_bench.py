"""bench.py itself: the plain run times exactly --steps steps and reports only the headline; --dump-outputs writes what
the last timed step computed, the same in every run with the same arguments, within its size budget."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way(tmp_path):
    import bench

    rs = np.random.RandomState(3)
    arrays = {"big": rs.rand(600, 500).astype(np.float32), "small": rs.rand(7), "ints": np.arange(5)}
    budget = 400_000
    for run in ("a", "b"):
        bench.dump_outputs(tmp_path / run, arrays, budget=budget)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["big.npy", "ints.npy", "small.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= budget
    small, ints = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "ints.npy")
    assert small.dtype == np.float64 and np.array_equal(small, arrays["small"])
    assert ints.dtype == np.float32 and np.array_equal(ints, np.arange(5, dtype=np.float32))
    big_a, big_b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert big_a.dtype == np.float32 and 0 < big_a.size < arrays["big"].size
    assert np.array_equal(big_a, big_b)  # a fixed sample: the same elements in every run
    assert np.isin(big_a, arrays["big"]).all()


def _plain_run(out_dir, steps=4, warmup=2, settle=200):
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--config", "c2", "--steps", str(steps), "--warmup",
           str(warmup), "--settle-steps", str(settle), "--dump-outputs", str(out_dir)]
    done = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-3000:]
    lines = [ln for ln in done.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, done.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_times_its_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    steps, warmup, settle = 4, 2, 200
    first = _plain_run(tmp_path / "a", steps, warmup, settle)
    second = _plain_run(tmp_path / "b", steps, warmup, settle)
    for out in (first, second):
        assert out["steps"] == steps and out["warmup"] == warmup and out["repeats"] == 1
        assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-9)
        assert out["higher_is_better"] is True and out["unit"] == "iters/s" and out["dtype"] == "f32"
        # the headline only: nothing that takes phases or runs of its own
        assert not {"roofline", "kernel_ms_per_step", "clock_mhz", "cpu_baseline", "general_psf"} & set(out)
        # warm-up + settle (the policy's epochs included) + the timed steps, whatever the policy decided
        assert out["check"]["epochs_run"] == warmup + settle + steps
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["flux_flux.npy", "loss_scalars.npy"]
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and np.isfinite(a).all()
        assert np.array_equal(a, b), name
    assert np.load(tmp_path / "a" / "flux_flux.npy").shape == (1024, 1024)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "loss_scalars.npy"),
                                  np.asarray(first["check"]["scalars_last_step"], dtype=np.float32))

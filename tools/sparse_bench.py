"""Times of the sparse point-source flux component: its two kernels, its whole optimizer step, and what it costs a fit.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/sparse_bench.py [--out FILE.json]

1. At --size^2 (2048) and N = 100, 1 000, 10 000 sources spread over the image: `jd_sparse_render` (zero fill + the
   (source, tap) kernel) and `jd_sparse_backward` from the library's kernel timers (hipEvent pairs around the launches),
   and the whole sparse step -- backward, the Adam step of the three vectors, render -- between two events on the
   stream, median over --repeats regions of --launches steps.  The render tests every tap against every source: its
   time grows with N^2 once the zero fill (4 bytes per pixel) no longer dominates.
2. The by-value step time of a --size^2, --obs observation joint fit of a diffuse component (uniform prior) with and
   without a points component of --fit-sources sources: interleaved regions of --steps epochs, wall clock around a
   synchronised region (as bench.py), median over --repeats rounds.
The shader clock the device holds under load (`_hip.clock_probe`) is recorded before and after.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

DEVICE = "cuda:0"


def sources(n, size, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.uniform(0.5, 5.0, n).astype(np.float32), rs.uniform(0, size - 1, n).astype(np.float32),
            rs.uniform(0, size - 1, n).astype(np.float32))


def kernel_times(size, counts, launches, repeats):
    from jolideco_amd import MAPDeconvolver, SparseSpatialFluxComponent, _hip
    from jolideco_amd.core import _SparseComponentState

    out = {}
    for n in counts:
        flux, x_pos, y_pos = sources(n, size)
        comp = SparseSpatialFluxComponent.from_numpy(flux=flux, x_pos=x_pos, y_pos=y_pos, shape=(size, size)).to(DEVICE)
        grad = torch.from_numpy(np.random.RandomState(1).normal(size=(size, size)).astype(np.float32)).to(DEVICE)
        state = _SparseComponentState("points", comp, grad, MAPDeconvolver(device=DEVICE, learning_rate=1e-4))
        step = 0
        for _ in range(10):
            step += 1
            state.step(step)
            state.cur = 1 - state.cur
        torch.cuda.synchronize()
        _hip.profile_enable(8 * launches)
        for _ in range(launches):
            step += 1
            state.step(step)
            state.cur = 1 - state.cur
        prof = _hip.profile_read()
        entry = {"sources": n}
        for timer in ("sparse_render", "sparse_backward", "adam"):
            total_ms, count = prof[timer]
            entry[f"{timer}_us"] = 1e3 * total_ms / max(count, 1)
            entry[f"{timer}_launches"] = int(count)
        regions = []
        for _ in range(repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                step += 1
                state.step(step)
                state.cur = 1 - state.cur
            end.record()
            end.synchronize()
            regions.append(1e3 * start.elapsed_time(end) / launches)
        entry["step_us"] = float(np.median(regions))
        entry["step_us_min_max"] = [float(min(regions)), float(max(regions))]
        out[str(n)] = entry
    return out


def fit_step_times(size, n_obs, n_sources, steps, warmup, repeats):
    from jolideco_amd import FluxComponents, MAPDeconvolver, SparseSpatialFluxComponent, SpatialFluxComponent
    from jolideco_amd.data import synthetic_observations

    sessions = {}
    for name in ("diffuse", "diffuse + points"):
        datasets, _, flux_init = synthetic_observations(shape=(size, size), n_obs=n_obs, seed=1)
        comps = FluxComponents()
        comps["diffuse"] = SpatialFluxComponent.from_numpy(flux=flux_init)
        if name != "diffuse":
            flux, x_pos, y_pos = sources(n_sources, size, seed=2)
            comps["points"] = SparseSpatialFluxComponent.from_numpy(flux=flux, x_pos=x_pos, y_pos=y_pos, shape=(size, size))
        deconvolver = MAPDeconvolver(n_epochs=1, display_progress=False, device=DEVICE, fit_mode="joint")
        deconvolver.use_graph = False  # by-value epochs for both (a session with a sparse component has no other form)
        session = deconvolver.session(datasets, components=comps)
        session._planned_ok = False
        for _ in range(warmup):
            session.epoch()
        sessions[name] = session
    torch.cuda.synchronize()
    times = {name: [] for name in sessions}
    for _ in range(repeats):
        for name, session in sessions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                session.epoch()
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - t0) / steps)
    return {name: {"step_us": float(np.median(v)), "step_us_min_max": [float(min(v)), float(max(v))]} for name, v in times.items()}


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, default=2048)
    parser.add_argument("--counts", type=int, nargs="+", default=[100, 1000, 10000])
    parser.add_argument("--launches", type=int, default=200)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--obs", type=int, default=4)
    parser.add_argument("--fit-sources", type=int, default=1000)
    parser.add_argument("--steps", type=int, default=100)
    parser.add_argument("--warmup", type=int, default=10)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    from jolideco_amd import _hip

    if not torch.cuda.is_available():
        raise SystemExit("sparse_bench.py measures on the GPU: no device found")
    result = {"device": torch.cuda.get_device_name(0), "size": args.size, "clock_mhz_before": _hip.clock_probe(device=DEVICE)}
    result["kernels"] = kernel_times(args.size, args.counts, args.launches, args.repeats)
    result["fit"] = dict(fit_step_times(args.size, args.obs, args.fit_sources, args.steps, args.warmup, args.repeats),
                         observations=args.obs, sources=args.fit_sources, fit_mode="joint")
    result["clock_mhz_after"] = _hip.clock_probe(device=DEVICE)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

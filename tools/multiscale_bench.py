"""Cost of `MultiScalePrior`: one pass (value + gradient) on a 2048^2 image with a K = 128 mixture of 8x8 patches, stride 4,
L = 3 levels, next to the plain `GMMPatchPrior` on the same image; and the two pyramid kernels' bytes over time.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/multiscale_bench.py [--out FILE.json] [--headline PARENT_LIBRARY]

A "pass" is one `device_fwd_bwd` call with a fresh draw.  The variants run INTERLEAVED in one process (boards differ by
several percent and drift with temperature): every round times one region of --steps calls of each (wall clock around a
synchronised region, as bench.py); the median over the rounds is reported with the shader clock the board holds under
load.  The kernels' times come from the library's timers (`jd_profile_*`: an event pair around every launch) in a run of
their own; their bytes are what the algorithm needs, from the shapes (`level_bytes`): every image read or written once,
the halo not counted -- against the 8 TB/s the other streaming kernels are held to.

--headline LIB: `bench.py --gpus 1 --steps 200 --warmup 20 --no-c6 --no-cpu-baseline` as child processes, the in-tree
library and LIB (a build of the parent commit, which lacks the jd_multiscale_* entries: the binding loads strictly, so
they are taken out of it for that process) alternating, --pairs times.  The headline fit has no such prior.
Nothing is gated on these numbers.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

SIZE, K, STRIDE, LEVELS = 2048, 128, 4, 3
NEW_EXPORTS = ("jd_multiscale_down", "jd_multiscale_up_adjoint", "jd_multiscale_value")
OLD_LIBRARY_RUNNER = (
    "import runpy, sys; from jolideco_amd import _hip; "
    f"[_hip.EXPORTS.pop(n) for n in {NEW_EXPORTS!r}]; "
    "[_hip.KERNEL_IDS.pop(n) for n in ('multiscale_down', 'multiscale_up')]; "
    "sys.argv = ['bench.py'] + sys.argv[1:]; runpy.run_path('bench.py', run_name='__main__')"
)


def level_bytes(H, W, n_levels):
    """(down, up) bytes the launches of one pass with gradient must move, every level evaluated: float32 images"""
    down = up = 0
    for level in range(n_levels):
        pooled = (H >> level) * (W >> level)
        last, first = level == n_levels - 1, level == 0
        down += 4 * (H * W + (0 if last else H * W) + 2 * pooled)           # read g_{l-1}; write g_l, d_l and the zeros of dd_l
        up += 4 * ((0 if last else H * W) + pooled + H * W * (2 if first else 1))  # read dg_l, dd_l; write (first: read + write)
    return down, up


def headline(parent_library, pairs):
    rows = []
    bench = ["--gpus", "1", "--steps", "200", "--warmup", "20", "--no-c6", "--no-cpu-baseline"]
    for pair in range(pairs):
        for name in ("parent", "child"):
            env = dict(os.environ)
            if name == "parent":
                env["JOLIDECO_HIP_LIBRARY"] = str(parent_library)
                cmd = [sys.executable, "-c", OLD_LIBRARY_RUNNER] + bench
            else:
                env.pop("JOLIDECO_HIP_LIBRARY", None)
                cmd = [sys.executable, "bench.py"] + bench
            done = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
            if done.returncode != 0:
                raise RuntimeError(f"bench.py ({name}) failed with {done.returncode}: {done.stderr[-2000:]}")
            line = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("{")][-1])
            rows.append({"pair": pair + 1, "library": name, "result": line})
            print(f"headline pair {pair + 1} {name}: {json.dumps(line)[:300]}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--size", type=int, default=SIZE)
    ap.add_argument("--headline", default=None, metavar="PARENT_LIBRARY")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {}
    if args.headline:  # (first: the child processes run alone on the device)
        result["headline"] = headline(Path(args.headline).resolve(), args.pairs)
    from jolideco_amd import GMMPatchPrior, MultiScalePrior, _hip
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    device = torch.device("cuda:0")
    size = args.size
    means, covs, weights = synthetic_gmm(K, 64, seed=0)
    gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=STRIDE))
    flux = torch.from_numpy(np.random.RandomState(0).gamma(20, size=(size, size)).astype(np.float32)).to(device)
    value, grad = torch.zeros(1, device=device), torch.zeros_like(flux)
    new_inner = lambda: GMMPatchPrior(gmm=gmm, stride=STRIDE, generator=torch.Generator().manual_seed(3))  # noqa: E731
    variants = {
        "gmm-patches": new_inner(),
        f"multiscale L={LEVELS}": MultiScalePrior(new_inner(), n_levels=LEVELS),
        "multiscale L=1": MultiScalePrior(new_inner(), n_levels=1),
    }

    def region(prior, steps):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(steps):
            prior.device_fwd_bwd(flux, value, grad=grad, coef=-1.0)
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) / steps

    for prior in variants.values():
        region(prior, args.warmup)
    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, prior in variants.items():  # interleaved: every round sees the same board state
            times[name].append(region(prior, args.steps))
    assert np.isfinite(float(value)) and bool(torch.isfinite(grad).all())
    result["workload"] = f"{size}^2, K = {K}, 8x8 patches, stride {STRIDE}"
    result["timing"] = f"median of {args.repeats} interleaved regions of {args.steps} passes (value + gradient)"
    result["us_per_pass"] = {name: 1e6 * float(np.median(t)) for name, t in times.items()}
    result["us_min_max"] = {name: [1e6 * float(np.min(t)), 1e6 * float(np.max(t))] for name, t in times.items()}

    # the two kernels alone: the library's timers around every launch, a run of its own
    prior = variants[f"multiscale L={LEVELS}"]
    passes = 20
    _hip.profile_enable(capacity=passes * 64)
    for _ in range(passes):
        prior.device_fwd_bwd(flux, value, grad=grad, coef=-1.0)
    timers = _hip.profile_read()
    down_bytes, up_bytes = level_bytes(size, size, LEVELS)
    result["kernels"] = {}
    for name, nbytes in (("multiscale_down", down_bytes), ("multiscale_up", up_bytes)):
        total_ms, launches = timers[name]
        assert launches == passes * LEVELS, (name, launches)
        us = 1e3 * total_ms / passes
        result["kernels"][name] = {"launches_per_pass": LEVELS, "us_per_pass": us, "bytes_per_pass": nbytes,
                                   "tb_per_s": nbytes / (us * 1e-6) / 1e12, "share_of_8_tb_per_s": nbytes / (us * 1e-6) / 8e12}
    result["shader_clock_mhz"] = _hip.clock_probe(5.0, device)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

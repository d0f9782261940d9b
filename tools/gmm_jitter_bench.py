"""Cost of `JitteredGMMPatchPrior` (the reference's `jitter=True`): one pass (value + gradient) of it and of the plain
`GMMPatchPrior` on the same handle, at 2048^2 with a K = 128 mixture of 8x8 patches at stride 4 and at 1024^2 with a K = 16
mixture of 16x16 patches at stride 8, and the two new kernels' bytes over time.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/gmm_jitter_bench.py [--out FILE.json] [--markdown FILE.md]
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python tools/gmm_jitter_bench.py --trace-passes 20
    timeout -k 10 60 python tools/gmm_jitter_bench.py --kernel-stats DIR --out FILE.json --markdown FILE.md   (no GPU needed)

A "pass" is one `device_fwd_bwd` call with a fresh draw.  The two variants share one mixture handle and run INTERLEAVED in
one process (boards differ by several percent and drift with temperature): every round times one region of --steps calls
of each (wall clock around a synchronised region, as bench.py); the median over the rounds is reported with the shader
clock the board holds under load.  The comparison is the plain pass.  The jittered prior adds the staging kernel and the
adjoint kernel and runs the SAME pass kernels on the staged image: at stride P / 2 that image has about 4 x the pixels of
the flux and about the same number of patches, at stride P instead of P / 2 -- so the pass itself may cost differently, and
"difference" below is everything: the two kernels, the small asynchronous copy of the draws, and the change of the pass.

The kernels' own times come from a kernel trace in a run of its own (--trace-passes: nothing but jittered passes at
2048^2; --kernel-stats reads the `kernels` view of the trace's `*_results.db`).  Their bytes are what the algorithm needs, from
the shape, with S = n_y P x n_x P floats: stage = read flux + write S + zero G = 4 HW + 8 S bytes; adjoint = read G + read and
write the gradient = 4 S + 8 HW bytes (identity norm) -- against the 8 TB/s the other streaming kernels are held to.  Nothing
is gated on these numbers.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

# size -> (components, features, stride)
WORKLOADS = {2048: (128, 64, 4), 1024: (16, 256, 8)}
SIZES = tuple(WORKLOADS)
KERNEL_BYTES = {"gmm_jitter_stage_kernel": (4, 8), "gmm_jitter_adjoint_kernel": (8, 4)}  # bytes per (flux pixel, pixel of S)
HBM_TB_PER_S = 8.0


def make_priors(size, seed=3):
    import torch

    from jolideco_amd import GMMPatchPrior, JitteredGMMPatchPrior
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    k, features, stride = WORKLOADS[size]
    means, covs, weights = synthetic_gmm(k, features, seed=0)
    gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=stride))
    new = lambda cls: cls(gmm=gmm, stride=stride, generator=torch.Generator().manual_seed(seed))  # noqa: E731
    return {"plain": new(GMMPatchPrior), "jitter": new(JitteredGMMPatchPrior)}


def staged_pixels(size):
    _, features, stride = WORKLOADS[size]
    patch = int(round(features**0.5))
    overlap = patch - stride
    n = len(range(overlap, size - stride - overlap, stride))
    return (n * patch) ** 2


def kernel_stats(directory, size):
    """{kernel: {us_per_launch, tb_per_s, share}} of the two new kernels from a kernel trace's database"""
    import sqlite3

    rows = {}
    for path in Path(directory).rglob("*_results.db"):  # (the profiler's default output: its `kernels` view, one row per launch)
        with sqlite3.connect(path) as db:
            for name in KERNEL_BYTES:
                calls, total = db.execute("select count(*), sum(duration) from kernels where name like ?", (f"%{name}%",)).fetchone()
                if calls:
                    entry = rows.setdefault(name, {"calls": 0, "total_ns": 0.0})
                    entry["calls"] += int(calls)
                    entry["total_ns"] += float(total)
    out = {}
    for name, entry in rows.items():
        us = 1e-3 * entry["total_ns"] / entry["calls"]
        nbytes = KERNEL_BYTES[name][0] * size * size + KERNEL_BYTES[name][1] * staged_pixels(size)
        tb = nbytes / (us * 1e-6) / 1e12
        out[name] = {"launches": entry["calls"], "us_per_launch": us, "bytes_per_launch": nbytes, "tb_per_s": tb,
                     "share_of_8_tb_per_s": tb / HBM_TB_PER_S}
    return out


def markdown(result):
    lines = ["| image | variant | us per pass (median) | min | max |", "|---|---|---|---|---|"]
    for size, entry in result.get("passes", {}).items():
        for name, us in entry["us_per_pass"].items():
            lo, hi = entry["us_min_max"][name]
            lines.append(f"| {size}^2 | {name} | {us:.1f} | {lo:.1f} | {hi:.1f} |")
        lines.append(f"| {size}^2 | difference | {entry['us_added']:.1f} | | |")
    if "shader_clock_mhz" in result:
        lines += ["", f"Shader clock under load: {result['shader_clock_mhz']:.0f} MHz."]
    if result.get("kernels"):
        lines += ["", "| kernel (2048^2) | launches | us per launch | bytes | TB/s | share of 8 TB/s |", "|---|---|---|---|---|---|"]
        for name, k in result["kernels"].items():
            lines.append(f"| `{name}` | {k['launches']} | {k['us_per_launch']:.1f} | {k['bytes_per_launch']} | {k['tb_per_s']:.2f} | "
                         f"{100 * k['share_of_8_tb_per_s']:.0f} % |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--trace-passes", type=int, default=0, help="only run this many jittered passes at 2048^2 (under a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="add the two kernels' figures from a kernel trace's output")
    ap.add_argument("--out", default=None)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    result = {}
    if args.out and Path(args.out).exists():
        result = json.loads(Path(args.out).read_text())
    if args.kernel_stats:
        result["kernels"] = kernel_stats(args.kernel_stats, SIZES[0])
    else:
        import torch

        from jolideco_amd import _hip

        device = torch.device("cuda:0")
        priors = {size: make_priors(size) for size in SIZES}
        images = {size: torch.from_numpy(np.random.RandomState(size).gamma(20, size=(size, size)).astype(np.float32)).to(device)
                  for size in SIZES}
        value = torch.zeros(1, device=device)
        grads = {size: torch.zeros_like(image) for size, image in images.items()}

        def region(prior, size, steps):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps):
                prior.device_fwd_bwd(images[size], value, grad=grads[size], coef=-1.0)
            torch.cuda.synchronize(device)
            return (time.perf_counter() - t0) / steps

        if args.trace_passes:
            region(priors[SIZES[0]]["jitter"], SIZES[0], args.trace_passes)
            return
        result["workload"] = {str(size): f"K = {k}, {int(round(f**0.5))}^2 patches, stride {s}, max mode, identity norm"
                              for size, (k, f, s) in WORKLOADS.items()}
        result["timing"] = f"median of {args.repeats} interleaved regions of {args.steps} passes (value + gradient)"
        result["passes"] = {}
        for size in SIZES:
            for prior in priors[size].values():
                region(prior, size, args.warmup)
            times = {name: [] for name in priors[size]}
            for _ in range(args.repeats):
                for name, prior in priors[size].items():  # interleaved: every round sees the same board state
                    times[name].append(region(prior, size, args.steps))
            assert np.isfinite(float(value)) and bool(torch.isfinite(grads[size]).all())
            us = {name: 1e6 * float(np.median(t)) for name, t in times.items()}
            result["passes"][str(size)] = {
                "us_per_pass": us, "us_min_max": {name: [1e6 * float(np.min(t)), 1e6 * float(np.max(t))] for name, t in times.items()},
                "us_added": us["jitter"] - us["plain"],
            }
        result["shader_clock_mhz"] = _hip.clock_probe(5.0, device)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    if args.markdown:
        Path(args.markdown).parent.mkdir(parents=True, exist_ok=True)
        Path(args.markdown).write_text(markdown(result))


if __name__ == "__main__":
    main()

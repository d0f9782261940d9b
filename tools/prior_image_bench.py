"""Cost of `GMMPatchPrior.prior_image_average`: time per draw at 2048^2 with a K = 128 mixture of 8x8 patches at stride 4
and with a K = 16 mixture of 16x16 patches at stride 8, beside the value-only pass of the same handle (`prior_fwd_bwd`
without a gradient -- the forward pass a draw starts with, which is the parent commit's code), and the two added launches'
bytes over time.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/prior_image_bench.py [--out FILE.json] [--markdown FILE.md]

A draw is one `GmmHandle.prior_image` call with a fresh roll, accumulated on the device; the two variants share one handle
and run INTERLEAVED in one process (wall clock around a synchronised region of --steps calls, as bench.py); the median over
the rounds is reported with the shader clock the board holds under load.  `prior_image_average(n)` is n such draws and one
copy of the image to the host; that copy is timed apart.

The added launches (`gmm_patch_mean_kernel`, `gmm_prior_image_gather_kernel`) are timed together by the library's own event
pairs (`_hip.profile_enable`; they run under the "gmm_gather" timer, which a value-only pass never starts) in a region of
its own.  Their bytes are what the algorithm needs, from the shape, with n patches: the normed flux read once for the means
(4 HW; its P^2 / s^2-fold re-reads are L2's), the accumulator read and written (8 HW), the table gathered once per
covering patch and pixel (4 HW P^2 / s^2, from L2 -- the table itself is K P^2 floats) and winner and mean per patch (8 n,
staged per tile) -- against the 8 TB/s the streaming kernels are held to.  Nothing is gated on these numbers.
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

# label -> (image edge, components, features, stride)
WORKLOADS = {"8x8": (2048, 128, 64, 4), "16x16": (2048, 16, 256, 8)}
HBM_TB_PER_S = 8.0


def added_bytes(size, features, stride):
    patch = int(round(features**0.5))
    n = ((size - patch) // stride + 1) ** 2
    cover = (patch // stride) ** 2
    return {"flux read for the means": 4 * size * size, "accumulator read + write": 8 * size * size,
            "table gathers (L2)": 4 * size * size * cover, "winner + mean per patch": 8 * n}


def markdown(result):
    lines = ["| workload | variant | us per call (median) | min | max |", "|---|---|---|---|---|"]
    for label, entry in result["draws"].items():
        for name, us in entry["us_per_call"].items():
            lo, hi = entry["us_min_max"][name]
            lines.append(f"| {label} | {name} | {us:.1f} | {lo:.1f} | {hi:.1f} |")
        lines.append(f"| {label} | difference | {entry['us_added']:.1f} | | |")
        lines.append(f"| {label} | copy of the image to the host, once per average | {entry['us_copy_to_host']:.1f} | | |")
    lines += ["", f"Shader clock under load: {result['shader_clock_mhz']:.0f} MHz.", "",
              "| workload | added launches, us per draw | bytes (all) | TB/s | share of 8 TB/s | bytes without the L2 gathers | share |",
              "|---|---|---|---|---|---|---|"]
    for label, k in result["added_launches"].items():
        lines.append(f"| {label} | {k['us_per_draw']:.1f} | {k['bytes']} | {k['tb_per_s']:.2f} | {100 * k['share_of_8_tb_per_s']:.0f} % | "
                     f"{k['bytes_hbm']} | {100 * k['share_hbm']:.0f} % |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()

    import torch

    from jolideco_amd import GMMPatchPrior, _hip
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    device = torch.device("cuda:0")
    result = {"workload": {}, "draws": {}, "added_launches": {},
              "timing": f"median of {args.repeats} interleaved regions of {args.steps} calls"}
    for label, (size, k, features, stride) in WORKLOADS.items():
        patch = int(round(features**0.5))
        result["workload"][label] = f"{size}^2, K = {k}, {patch}^2 patches, stride {stride}, identity norm"
        means, covs, weights = synthetic_gmm(k, features, seed=0)
        gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=stride))
        prior = GMMPatchPrior(gmm=gmm, stride=stride, generator=torch.Generator().manual_seed(3))
        handle = gmm.handle(device)
        image = torch.from_numpy(np.random.RandomState(size).gamma(20, size=(size, size)).astype(np.float32)).to(device)
        table = handle.prior_image_table(gmm.eigen_images)
        out, value = torch.zeros_like(image), torch.zeros(1, device=device)

        def draw():
            handle.prior_image(image, stride, prior.draw_shifts(image.shape), table, out, scale=1.0 / args.steps, accumulate=True)

        def value_only():
            handle.prior_fwd_bwd(image, stride, prior.draw_shifts(image.shape), value, 1.0)

        def region(call, steps):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            torch.cuda.synchronize(device)
            return (time.perf_counter() - t0) / steps

        calls = {"value-only pass": value_only, "prior image draw": draw}
        for call in calls.values():
            region(call, args.warmup)
        times = {name: [] for name in calls}
        for _ in range(args.repeats):
            for name, call in calls.items():  # interleaved: every round sees the same board state
                times[name].append(region(call, args.steps))
        assert bool(torch.isfinite(out).all()) and np.isfinite(float(value))
        copies = [region(lambda: out.cpu(), 1) for _ in range(5)]
        us = {name: 1e6 * float(np.median(t)) for name, t in times.items()}
        result["draws"][label] = {
            "us_per_call": us, "us_min_max": {name: [1e6 * float(np.min(t)), 1e6 * float(np.max(t))] for name, t in times.items()},
            "us_added": us["prior image draw"] - us["value-only pass"], "us_copy_to_host": 1e6 * float(np.median(copies)),
        }
        _hip.profile_enable(4096)
        region(draw, args.steps)
        total_ms, launches = _hip.profile_read()["gmm_gather"]
        assert launches == args.steps, f"{launches} timed scopes for {args.steps} draws"
        us_added = 1e3 * total_ms / launches
        parts = added_bytes(size, features, stride)
        nbytes = sum(parts.values())
        hbm = nbytes - parts["table gathers (L2)"]
        result["added_launches"][label] = {
            "us_per_draw": us_added, "bytes_by_part": parts, "bytes": nbytes, "tb_per_s": nbytes / (us_added * 1e-6) / 1e12,
            "share_of_8_tb_per_s": nbytes / (us_added * 1e-6) / 1e12 / HBM_TB_PER_S, "bytes_hbm": hbm,
            "share_hbm": hbm / (us_added * 1e-6) / 1e12 / HBM_TB_PER_S,
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

"""Time of the 16x16 (256-feature) GMM patch prior pass: 512^2 image, K = 200 components, stride 8 -- the reference's
16x16 mixture's size -- in arg-max and in logsumexp mode, value only and value + gradient.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/gmm16_bench.py [--out FILE.json]

A "pass" is one `jd_gmm_prior_fwd_bwd` call of the whole prior with a fresh pair of cycle-spin shifts.  The four
variants run INTERLEAVED in one process (boards differ by several percent and drift with temperature): every round times
one region of --steps calls of each (wall clock around a synchronised region, as bench.py); the median over the rounds
is reported with the shader clock the board holds under load.
Roof: the exact-fp32 matrix instruction runs at 64 FLOP per clock and SIMD, 256 per CU.  Forward FLOPs = patches x K x
2 x 256^2 x 1/2 (the triangle of the factor).  The backward pass recomputes y and multiplies by the factor once more,
twice the forward count per (patch, component) it visits: all K in logsumexp mode; in arg-max mode the distinct winners
of each tile (16 or 32 patches: 32 once that gives every compute unit a block), counted here from the arg-max the
library returns.  The gradient variants' backward time is the difference to the value-only variant (it includes the
overlap-add).  Nothing is gated on these numbers.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--components", type=int, default=200)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import GMMPatchPrior, _hip
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    device = torch.device("cuda:0")
    shape = (args.size, args.size)
    means, covs, weights = synthetic_gmm(args.components, 256, seed=0)
    gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=args.stride))
    flux = torch.from_numpy(np.random.RandomState(0).gamma(20, size=shape).astype(np.float32)).to(device)
    value, grad = torch.zeros(1, device=device), torch.zeros_like(flux)
    variants = {}
    for mode, marginalize in (("max", False), ("lse", True)):
        prior = GMMPatchPrior(gmm=gmm, stride=args.stride, marginalize=marginalize, generator=torch.Generator().manual_seed(3))
        variants[f"{mode}_value"] = (prior, None)
        variants[f"{mode}_value_gradient"] = (prior, grad)

    def region(prior, g, steps):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(steps):
            prior.device_fwd_bwd(flux, value, grad=g, coef=-1.0)
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) / steps

    for prior, g in variants.values():
        region(prior, g, args.warmup)
    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, (prior, g) in variants.items():  # interleaved: every round sees the same board state
            times[name].append(region(prior, g, args.steps))
    clock = _hip.clock_probe(5.0, device)

    n_py = (shape[0] - 16) // args.stride + 1
    n_px = (shape[1] - 16) // args.stride + 1
    n = n_py * n_px
    arg = torch.zeros(n, dtype=torch.int32, device=device)
    gmm.handle(device).prior_fwd_bwd(flux, args.stride, (0, 0), value, 1.0, argmax_out=arg)
    torch.cuda.synchronize(device)
    winners = arg.cpu().numpy()
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    tile = 32 if (n + 31) // 32 >= n_cu else 16  # patches per block (gmm256.hip: tile_halves)
    visits = sum(len(set(winners[i : i + tile].tolist()) - {-1}) * tile for i in range(0, n, tile))
    pair = 2.0 * 256 * 256 * 0.5  # FLOPs of one triangular product per (patch, component)
    flops = {"forward": n * args.components * pair, "backward_lse": 2 * n * args.components * pair,
             "backward_max": 2 * visits * pair}
    roof = n_cu * 256 * clock * 1e6  # FLOP/s of the fp32 matrix instruction at the measured clock
    med = {name: float(np.median(t)) for name, t in times.items()}
    result = {"workload": f"GMM patch prior pass, 16x16 patches, {args.size}^2, K = {args.components}, stride {args.stride}",
              "timing": f"median of {args.repeats} interleaved regions of {args.steps} calls", "shader_clock_mhz": clock,
              "compute_units": n_cu, "fp32_mfma_roof_tflops": roof / 1e12, "patches": n, "patches_per_block": tile, "tiles": (n + tile - 1) // tile,
              "flops": flops, "variants": {}}
    for name in variants:
        result["variants"][name] = {"us_per_pass": 1e6 * med[name], "us_min": 1e6 * float(np.min(times[name])),
                                    "us_max": 1e6 * float(np.max(times[name]))}
    for mode in ("max", "lse"):
        fwd, bwd = med[f"{mode}_value"], med[f"{mode}_value_gradient"] - med[f"{mode}_value"]
        result[f"{mode}_forward_roof_fraction"] = flops["forward"] / fwd / roof
        result[f"{mode}_backward_us"] = 1e6 * bwd
        result[f"{mode}_backward_roof_fraction"] = flops[f"backward_{mode}"] / bwd / roof if bwd > 0 else None
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

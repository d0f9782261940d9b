"""Cost of an image norm on the GMM patch prior step: identity against asinh at 2048^2, K = 128.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/image_norm_bench.py [--out FILE.json]

The "prior step" is one `jd_gmm_prior_fwd_bwd` call of the whole prior (value + gradient accumulated into an image,
stride 4, arg-max mode, a fresh pair of cycle-spin shifts per call).  Under a norm the call runs one more kernel, the
streaming n(flux) pass (H W 4 bytes read + as many written), and its gather multiplies by n'(raw flux) (H W 4 bytes more
read).  Boards differ by several percent and drift with temperature, so the two variants run INTERLEAVED in one
process: every round times one region of --steps calls of each (wall clock around a synchronised region, as bench.py);
the median over 9 rounds is reported, with the shader clock the board holds under load.
The two variants do NOT do the same work behind the norm (the mixture sees other pixel values, the screen keeps another
number of components per patch), so the difference is the cost of a norm on this step, not the time of the extra pass.
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
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import GMMPatchPrior, _hip
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
    from jolideco_amd.utils.norms import ASinhImageNorm, IdentityImageNorm

    device = torch.device("cuda:0")
    shape = (args.size, args.size)
    means, covs, weights = synthetic_gmm(args.components, 64, seed=0)
    flux = torch.from_numpy(np.random.RandomState(0).gamma(20, size=shape).astype(np.float32)).to(device)
    variants = {}
    for name, norm in (("identity", IdentityImageNorm()), ("asinh", ASinhImageNorm(alpha=3.0, beta=40.0))):
        gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))  # a handle each
        variants[name] = GMMPatchPrior(gmm=gmm, norm=norm, generator=torch.Generator().manual_seed(3))
    value, grad = torch.zeros(1, device=device), torch.zeros_like(flux)

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
    clock = _hip.clock_probe(5.0, device)
    result = {"workload": f"GMM patch prior step, {args.size}^2, K = {args.components}, stride 4, arg-max mode",
              "timing": f"median of {args.repeats} interleaved regions of {args.steps} calls", "shader_clock_mhz": clock,
              "image_bytes": 4 * shape[0] * shape[1], "variants": {}}
    for name in variants:
        result["variants"][name] = {"us_per_step": 1e6 * float(np.median(times[name])), "us_min": 1e6 * float(np.min(times[name])),
                                    "us_max": 1e6 * float(np.max(times[name]))}
    result["asinh_minus_identity_us"] = result["variants"]["asinh"]["us_per_step"] - result["variants"]["identity"]["us_per_step"]
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

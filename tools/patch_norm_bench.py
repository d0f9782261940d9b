"""Cost of the standardized patch norm: one GMM patch prior pass (value + gradient, arg-max and logsumexp mode) under
`StandardizedSubtractMeanPatchNorm` against the dense subtract-mean pass at the same shape.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/patch_norm_bench.py [--out FILE.json]

  D = 64:  1024^2 image, K = 128 components, stride 4;     D = 256:  512^2 image, K = 200 components, stride 8.
A "pass" is one `device_fwd_bwd` call of the whole prior with a fresh pair of cycle-spin shifts.  The standardized norm
always takes the dense fp32 kernels, so its baseline is the dense subtract-mean pass: the screens are switched off for
the whole process (JD_GMM_SCREEN = 0, JD_GMM_LSE_SCREEN = 0; D = 256 has no screen).  All variants run INTERLEAVED in one
process (boards differ by several percent and drift with temperature): every round times one region of --steps calls of
each (wall clock around a synchronised region, as bench.py); the median over the rounds is reported with the shader
clock the board holds under load.

--baseline-only times the subtract-mean variants alone and calls neither jd_gmm_set_patch_norm nor
jd_gmm_set_const_residual, so that it also runs on a library built from the commit before the norm (the binding loads
strictly: the entries are taken out of it):
    JOLIDECO_HIP_LIBRARY=jolideco_amd/libjolideco_hip_parent.so python tools/patch_norm_bench.py --baseline-only
Nothing is gated on these numbers.
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

SHAPES = {64: (1024, 128, 4), 256: (512, 200, 8)}  # D -> (image edge, components, stride)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--features", type=int, nargs="+", default=[64, 256], choices=[64, 256])
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import GMMPatchPrior, _hip, ops
    from jolideco_amd.data import synthetic_gmm
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
    from jolideco_amd.utils.norms import StandardizedSubtractMeanPatchNorm, SubtractMeanPatchNorm

    if args.baseline_only:
        for name in ("jd_gmm_set_patch_norm", "jd_gmm_set_const_residual"):
            _hip.EXPORTS.pop(name, None)
        ops.GmmHandle.set_patch_norm = lambda self, patch_norm: None
        GaussianMixtureModel.const_float64_numpy = None  # (no residual of the constants is handed over)
    _hip.set_option("JD_GMM_SCREEN", 0)
    _hip.set_option("JD_GMM_LSE_SCREEN", 0)
    device = torch.device("cuda:0")
    norms = {"subtract-mean": SubtractMeanPatchNorm()}
    if not args.baseline_only:
        norms["std-subtract-mean"] = StandardizedSubtractMeanPatchNorm()
    result = {"timing": f"median of {args.repeats} interleaved regions of {args.steps} passes (value + gradient), screens off",
              "library": _hip.lib()._name, "cases": {}}
    for d in args.features:
        size, k, stride = SHAPES[d]
        means, covs, weights = synthetic_gmm(k, d, seed=0)
        gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=stride))
        flux = torch.from_numpy(np.random.RandomState(0).gamma(20, size=(size, size)).astype(np.float32)).to(device)
        value, grad = torch.zeros(1, device=device), torch.zeros_like(flux)
        variants = {}
        for mode, marginalize in (("max", False), ("lse", True)):
            for name, norm in norms.items():
                variants[f"{mode}/{name}"] = GMMPatchPrior(gmm=gmm, stride=stride, marginalize=marginalize, patch_norm=norm,
                                                           generator=torch.Generator().manual_seed(3))

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
        case = {"workload": f"{size}^2, K = {k}, stride {stride}", "us_per_pass": {}, "us_min_max": {}}
        for name, t in times.items():
            case["us_per_pass"][name] = 1e6 * float(np.median(t))
            case["us_min_max"][name] = [1e6 * float(np.min(t)), 1e6 * float(np.max(t))]
        if not args.baseline_only:
            case["ratio_std_over_subtract_mean"] = {
                mode: case["us_per_pass"][f"{mode}/std-subtract-mean"] / case["us_per_pass"][f"{mode}/subtract-mean"] for mode in ("max", "lse")}
        result["cases"][f"D={d}"] = case
        del variants, gmm
    result["shader_clock_mhz"] = _hip.clock_probe(5.0, device)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

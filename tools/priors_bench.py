"""Kernel times of the point-source-layer priors and what the sub-pixel option costs a fit step.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/priors_bench.py [--out FILE.json]

1. At --size^2 (2048), from the library's kernel timers (hipEvent pairs around each launch): the sub-pixel kernel of the
   sparse priors beside the plain `elementwise_prior_kernel` (both move 12 B/pixel: flux read, gradient read and written),
   and the epilogue of the smoothness prior behind its convolution (16 B/pixel: flux and K (*) flux read, gradient read
   and written), each with its fraction of the 8 TB/s HBM roof.  The three images of a 2048^2 case (48 MiB)
   fit the 256 MiB Infinity Cache, so a fraction near or above 1 says the pass ran from cache, not that the roof is wrong;
   --size 8192 (768 MiB) measures HBM.
2. Step time of a --fit-size^2 (1024), 4-observation, two-component joint fit -- a GMM 8 x 8 prior on one layer, an
   inverse-gamma prior on the other -- with `cycle_spin_subpix` off and on: interleaved regions of --steps epochs, wall
   clock around a synchronised region (as bench.py), median over --repeats rounds, under the default epoch policy.
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

HBM_PEAK_GBS = 8000.0  # as bench.py


def kernel_times(size, launches):
    from jolideco_amd import ExponentialPrior, InverseGammaPrior, SmoothnessPrior, _hip

    device = torch.device("cuda:0")
    flux = torch.from_numpy(np.random.RandomState(0).gamma(2.0, size=(size, size)).astype(np.float32) + 0.05).to(device)
    value, grad = torch.zeros(1, device=device), torch.zeros_like(flux)
    generator = torch.Generator().manual_seed(3)
    variants = {
        "inverse-gamma": (InverseGammaPrior(), "elementwise_prior"),
        "inverse-gamma, cycle_spin_subpix": (InverseGammaPrior(cycle_spin_subpix=True, generator=generator), "elementwise_subpix"),
        "exponential": (ExponentialPrior(), "elementwise_prior"),
        "exponential, cycle_spin_subpix": (ExponentialPrior(cycle_spin_subpix=True, generator=generator), "elementwise_subpix"),
        "smoothness (width 2) epilogue": (SmoothnessPrior(), "smoothness"),
    }
    out = {}
    for name, (prior, timer) in variants.items():
        nbytes = (16 if timer == "smoothness" else 12) * size * size
        for _ in range(20):
            prior.device_fwd_bwd(flux, value, grad=grad, coef=-1e-3)
        torch.cuda.synchronize(device)
        _hip.profile_enable(4 * launches)
        for _ in range(launches):
            prior.device_fwd_bwd(flux, value, grad=grad, coef=-1e-3)
        prof = _hip.profile_read()
        total_ms, count = prof[timer]
        us = 1e3 * total_ms / max(count, 1)
        entry = {"kernel": _hip.lib().jd_kernel_name(_hip.KERNEL_IDS[timer]).decode(), "launches": int(count),
                 "us_per_launch": us, "bytes": nbytes, "gbs": nbytes / (us * 1e-6) / 1e9,
                 "fraction_of_hbm_roof": nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS}
        if timer == "smoothness":
            conv = {k: 1e3 * v[0] / v[1] for k, v in prof.items() if v[1] and k != timer}
            entry["convolution_us"] = conv
        out[name] = entry
    return out


def fit_step_times(size, n_obs, steps, warmup, repeats):
    from jolideco_amd import FluxComponents, GMMPatchPrior, InverseGammaPrior, MAPDeconvolver, SpatialFluxComponent
    from jolideco_amd.data import gaussian_kernel, synthetic_gmm, synthetic_observations
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    means, covs, weights = synthetic_gmm(128, 64, seed=0)
    sessions = {}
    for name, option in (("off", False), ("on", True)):
        datasets, _, flux_init = synthetic_observations(shape=(size, size), n_obs=n_obs, seed=1)
        for i, d in enumerate(datasets.values()):
            d["psf"] = {"extended": d["psf"], "points": gaussian_kernel(1.0 + 0.1 * i, (9, 9)).astype(np.float32)}
        gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))
        comps = FluxComponents()
        comps["extended"] = SpatialFluxComponent.from_numpy(flux=flux_init, prior=GMMPatchPrior(gmm=gmm))
        comps["points"] = SpatialFluxComponent.from_numpy(flux=0.05 * flux_init, prior=InverseGammaPrior(cycle_spin_subpix=option))
        deco = MAPDeconvolver(n_epochs=1, display_progress=False, device="cuda:0", fit_mode="joint")
        sessions[name] = deco.session(datasets, components=comps)

    def region(session, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            session.epoch()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for session in sessions.values():
        region(session, warmup)
    times = {name: [] for name in sessions}
    for _ in range(repeats):
        for name, session in sessions.items():
            times[name].append(region(session, steps))
    out = {name: {"us_per_step": 1e6 * float(np.median(t)), "us_min": 1e6 * float(np.min(t)), "us_max": 1e6 * float(np.max(t)),
                  "epoch_policy": sessions[name].graph_policy} for name, t in times.items()}
    out["on_minus_off_us"] = out["on"]["us_per_step"] - out["off"]["us_per_step"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--fit-size", type=int, default=1024)
    ap.add_argument("--observations", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernels-only", action="store_true", help="skip the fit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import _hip

    result = {"kernels": {"size": args.size, "timing": f"library timers, mean of {args.launches} launches",
                          "variants": kernel_times(args.size, args.launches)},
              "fit": None if args.kernels_only else {"workload": f"{args.fit_size}^2, {args.observations} observations, joint, GMM K = 128 + inverse-gamma",
                      "timing": f"median of {args.repeats} interleaved regions of {args.steps} epochs",
                      "variants": fit_step_times(args.fit_size, args.observations, args.steps, args.warmup, args.repeats)},
              "shader_clock_mhz": _hip.clock_probe(5.0, torch.device("cuda:0"))}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

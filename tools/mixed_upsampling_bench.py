"""Step time of a two-component joint fit whose components have DIFFERENT up-sampling factors, against today's only
other way to run such a model: both components at the finer grid.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 600 python tools/mixed_upsampling_bench.py [--out FILE.json]

Workload: 1024^2 counts, 4 observations, joint mode; "extended" under a K = 128 GMM patch prior (Gaussian 17-tap PSFs),
"points" under InverseGammaPrior (general 9x9 PSFs).  Factor pairs (extended, points) = (1, 2), (2, 1) and (2, 2).
Boards differ by several percent and drift with temperature, so the variants run INTERLEAVED in one process: every
round times one region of --steps epochs of each variant (wall clock around a synchronised region, as bench.py); the
median over --repeats rounds is reported.  A second, untimed phase brackets the library's kernels with event pairs and
reports the mixed Poisson launch alone, with its fraction of 8 TB/s from the algorithmic bytes
4 * (2 + sum_c 2 u_c^2) per counts pixel, and the shader clock the board holds under load.
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

PAIRS = ((1, 2), (2, 1), (2, 2))
HBM_PEAK = 8.0e12  # B/s, MI355X


def build_session(shape, n_obs, pair, device):
    from jolideco_amd import FluxComponents, GMMPatchPrior, InverseGammaPrior, MAPDeconvolver, SpatialFluxComponent
    from jolideco_amd.data import instrument_like_psf, synthetic_gmm, synthetic_observations
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    datasets, _, flux_init = synthetic_observations(shape=shape, n_obs=n_obs, seed=0)
    for i, d in enumerate(datasets.values()):
        d["psf"] = {"extended": d["psf"], "points": instrument_like_psf(i, (9, 9))}
    means, covs, weights = synthetic_gmm(128, 64, seed=0)
    gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=4))
    init_pts = np.random.RandomState(5).gamma(2, size=shape) * 0.2
    comps = FluxComponents()
    comps["extended"] = SpatialFluxComponent.from_numpy(
        flux=flux_init, upsampling_factor=pair[0], prior=GMMPatchPrior(gmm=gmm, generator=torch.Generator().manual_seed(3))
    )
    comps["points"] = SpatialFluxComponent.from_numpy(flux=init_pts, upsampling_factor=pair[1],
                                                      prior=InverseGammaPrior(alpha=10, beta=1.5))
    deco = MAPDeconvolver(n_epochs=1, display_progress=False, device=device, fit_mode="joint")
    return deco.session(datasets, components=comps)


def region(session, steps, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        session.epoch()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--obs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=60, help="untimed epochs per variant (the graph policy settles in them)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import _hip

    device = torch.device("cuda:0")
    shape = (args.size, args.size)
    sessions = {pair: build_session(shape, args.obs, pair, device) for pair in PAIRS}
    for session in sessions.values():
        region(session, args.warmup, device)
    times = {pair: [] for pair in PAIRS}
    for _ in range(max(args.repeats, 5)):
        for pair, session in sessions.items():  # interleaved: every round sees the same board state
            times[pair].append(region(session, args.steps, device))
    clock = _hip.clock_probe(5.0, device)
    result = {"workload": f"{args.size}^2 counts x {args.obs} observations, joint, GMM K=128 + inverse-gamma",
              "timing": f"median of {len(times[PAIRS[0]])} interleaved regions of {args.steps} steps", "shader_clock_mhz": clock,
              "variants": {}}
    for pair, session in sessions.items():
        result["variants"][str(pair)] = {
            "ms_per_step": 1e3 * float(np.median(times[pair])), "ms_per_step_min": 1e3 * float(np.min(times[pair])),
            "ms_per_step_max": 1e3 * float(np.max(times[pair])), "graph_policy": session.graph_policy,
            "methods": [[m.plan.method for m in models.values()] for models in session.total_loss.poisson_loss.npred_models_all][0],
        }
    # the kernels alone (event pairs on the stream; epochs run by value while the timers are on)
    for pair, session in sessions.items():
        _hip.profile_enable(8192)
        for _ in range(10):
            session.epoch()
        torch.cuda.synchronize(device)
        prof = _hip.profile_read()
        entry = result["variants"][str(pair)]
        entry["kernels_us"] = {k: round(1e3 * ms / n, 2) for k, (ms, n) in prof.items() if n}
        if prof["poisson_mixed"][1]:
            us = 1e3 * prof["poisson_mixed"][0] / prof["poisson_mixed"][1]
            bytes_ = 4.0 * (2 + sum(2 * u * u for u in pair)) * shape[0] * shape[1]
            entry["poisson_mixed_us"] = us
            entry["poisson_mixed_bytes"] = bytes_
            entry["poisson_mixed_fraction_of_8TBs"] = bytes_ / (us * 1e-6) / HBM_PEAK
    base = result["variants"][str((2, 2))]["ms_per_step"]
    for pair in PAIRS:
        result["variants"][str(pair)]["step_time_over_2_2"] = result["variants"][str(pair)]["ms_per_step"] / base
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

"""Cost of the optimizer step with options: jd_optimizer_step against jd_adam_step / jd_sgd_step on the same images.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/optimizer_options_bench.py [--out FILE.json] [--fit]

Step kernels at 2048^2, log flux, no mask -- streaming kernels bound by HBM, so the yardstick is bytes per pixel:
    adam            jd_adam_step                        36 B  (theta, flux, grad, m, v in; theta, flux, m, v out)
    adam-off        jd_optimizer_step, no option        36 B  (the same arithmetic in the new kernel family)
    adam-amsgrad    jd_optimizer_step, amsgrad          44 B  (+ max_exp_avg_sq in and out): 1.22 x adam by bytes
    sgd             jd_sgd_step                         20 B
    sgd-momentum    jd_optimizer_step, momentum 0.9     28 B  (+ momentum_buffer in and out): 1.40 x sgd by bytes
Boards differ by several percent and drift with temperature, so the variants run ALTERNATING in one process after a
warm-up; each launch is bracketed by device events, and the median over --repeats rounds of --steps launches is
reported.  The images (16 MiB each, 80 to 176 MiB per variant) do not fit the 256 MiB last-level cache together with the
other variants' between two launches of one variant; what one launch leaves there for the next of ITS OWN is the same
for every variant.
--fit: also the headline fit of bench.py (2048^2, 8 observations, GMM prior K = 128, joint) with
optimizer_kwargs={"amsgrad": True} beside the same fit under JOLIDECO_NO_FUSED_STEP=1, which has the same launch structure
(prior into the gradient image, then a stand-alone step): iterations/s of both from this one process, alternating.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

BYTES = {"adam": 36, "adam-off": 36, "adam-amsgrad": 44, "sgd": 20, "sgd-momentum": 28}


def step_variants(n, device):
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, stream_ptr
    from jolideco_amd.ops import adam_bias_terms

    lib = _hip.lib()
    rs = np.random.RandomState(0)
    new = lambda a: torch.from_numpy(a.astype(np.float32)).to(device)  # noqa: E731
    lr, beta1, beta2, eps = 1e-3, 0.9, 0.999, 1e-8
    step_size, bias2_sqrt = adam_bias_terms(10, lr, beta1, beta2)
    stream = stream_ptr(device)

    def images(adam, third):
        theta = rs.normal(size=n)
        out = {"theta": new(theta), "flux_in": new(np.exp(theta)), "flux_out": new(np.zeros(n)), "grad": new(rs.normal(size=n))}
        if adam:
            out["m"], out["v"] = new(0.1 * rs.normal(size=n)), new(rs.uniform(size=n) ** 2)
        if third:
            out["third"] = new(rs.uniform(size=n) ** 2)
        return out

    def options(kind, **fields):
        return _hip.OptimizerOptions(kind=kind, step_size=step_size, beta1=beta1, beta2=beta2, one_minus_beta1=1 - beta1,
                                     one_minus_beta2=1 - beta2, bias2_sqrt=bias2_sqrt, eps=eps, lr=lr, **fields)

    def plain_adam(im):
        return lambda: check(lib.jd_adam_step(ptr(im["theta"]), ptr(im["flux_in"]), ptr(im["flux_out"]), ptr(im["grad"]), ptr(im["m"]),
                                              ptr(im["v"]), None, n, step_size, beta1, beta2, 1 - beta1, 1 - beta2, bias2_sqrt, eps, 0, 1,
                                              None, stream))

    def plain_sgd(im):
        return lambda: check(lib.jd_sgd_step(ptr(im["theta"]), ptr(im["flux_in"]), ptr(im["flux_out"]), ptr(im["grad"]), None, n, lr, 0, 1,
                                             stream))

    def optioned(im, args, vmax=None, buf=None):
        return lambda: check(lib.jd_optimizer_step(ptr(im["theta"]), ptr(im["flux_in"]), ptr(im["flux_out"]), ptr(im["grad"]),
                                                   ptr(im.get("m")), ptr(im.get("v")), ptr(vmax), ptr(buf), None, n, ctypes.byref(args), 0, 1,
                                                   None, stream))

    a, b, c, d, e = images(True, False), images(True, False), images(True, True), images(False, False), images(False, True)
    keep = [a, b, c, d, e]
    return keep, {
        "adam": plain_adam(a),
        "adam-off": optioned(b, options(_hip.OPTIMIZER_ADAM)),
        "adam-amsgrad": optioned(c, options(_hip.OPTIMIZER_ADAM, amsgrad=1), vmax=c["third"]),
        "sgd": plain_sgd(d),
        "sgd-momentum": optioned(e, options(_hip.OPTIMIZER_SGD, momentum=0.9), buf=e["third"]),
    }


def time_steps(variants, steps, warmup, repeats, device):
    for _ in range(warmup):
        for call in variants.values():
            call()
    torch.cuda.synchronize(device)
    rounds = {name: [] for name in variants}
    for _ in range(repeats):
        pairs = {name: [] for name in variants}
        for _ in range(steps):
            for name, call in variants.items():  # (alternating: a drift of the board hits every variant alike)
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                call()
                end.record()
                pairs[name].append((start, end))
        torch.cuda.synchronize(device)
        for name, events in pairs.items():
            rounds[name].append(float(np.median([s.elapsed_time(e) for s, e in events])) * 1e3)
    return {name: float(np.median(values)) for name, values in rounds.items()}, {name: (min(v), max(v)) for name, v in rounds.items()}


def fit_sessions(device):
    """The headline fit twice: an option on, and no option under JOLIDECO_NO_FUSED_STEP=1 (read when a session is built)."""
    import bench
    from jolideco_amd import GMMPatchPrior, MAPDeconvolver, SpatialFluxComponent
    from jolideco_amd.data import synthetic_gmm, synthetic_observations
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta

    H, W, n_obs, K = bench.CONFIGS["c3"]
    sessions = {}
    for name, kwargs, env in (("amsgrad", {"amsgrad": True}, None), ("no-fused-step", None, "1")):
        if env is None:
            os.environ.pop("JOLIDECO_NO_FUSED_STEP", None)
        else:
            os.environ["JOLIDECO_NO_FUSED_STEP"] = env
        # (bench.build_session("c3", ...) with `optimizer_kwargs`: the same data, mixture and component)
        datasets, _, flux_init = synthetic_observations(shape=(H, W), n_obs=n_obs, seed=0)
        means, covs, weights = synthetic_gmm(K, bench.D, seed=0)
        gmm = GaussianMixtureModel.from_numpy(means, covs, weights, meta=GaussianMixtureModelMeta(stride=bench.STRIDE))
        comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=GMMPatchPrior(gmm=gmm))
        deconvolver = MAPDeconvolver(n_epochs=1, display_progress=False, device=device, fit_mode="joint", optimizer_kwargs=kwargs)
        sessions[name] = deconvolver.session(datasets, components=comp)
    os.environ.pop("JOLIDECO_NO_FUSED_STEP", None)
    return sessions


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import _hip

    device = torch.device("cuda:0")
    n = args.size * args.size
    keep, variants = step_variants(n, device)
    medians, spread = time_steps(variants, args.steps, args.warmup, args.repeats, device)
    result = {"size": args.size, "clock_mhz": _hip.clock_probe(device=device), "steps_us": medians, "steps_us_min_max": spread,
              "gb_per_s": {name: BYTES[name] * n / (us * 1e-6) / 1e9 for name, us in medians.items()},
              "amsgrad_over_adam": medians["adam-amsgrad"] / medians["adam"], "amsgrad_over_adam_by_bytes": 44 / 36,
              "momentum_over_sgd": medians["sgd-momentum"] / medians["sgd"], "momentum_over_sgd_by_bytes": 28 / 20,
              "off_over_adam": medians["adam-off"] / medians["adam"]}
    del keep
    if args.fit:
        result["fit"] = time_fits(device)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


def time_fits(device, epochs=30, warmup=25, repeats=5):
    import bench

    sessions = fit_sessions(device)
    for session in sessions.values():
        for _ in range(warmup):
            session.epoch()
        bench.warm_policy(session)  # (the "auto" policy's probe and trial epochs belong into no timed region)
    torch.cuda.synchronize(device)
    rates = {name: [] for name in sessions}
    for _ in range(repeats):
        for name, session in sessions.items():
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(epochs):
                session.epoch()
            torch.cuda.synchronize(device)
            rates[name].append(epochs / (time.perf_counter() - t0))
    return {"iterations_per_s": {name: float(np.median(v)) for name, v in rates.items()},
            "policy": {name: session.graph_policy for name, session in sessions.items()}}


if __name__ == "__main__":
    main()

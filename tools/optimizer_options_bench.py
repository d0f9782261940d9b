"""Cost of the optimizer step with options: jd_optimizer_step against jd_adam_step / jd_sgd_step on the same images.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 300 python tools/optimizer_options_bench.py [--out FILE.json] [--fit]

Step kernels at 2048^2, log flux, no mask -- streaming kernels bound by HBM, so the yardstick is bytes per pixel:
    adam            jd_adam_step                        36 B  (theta, flux, grad, m, v in; theta, flux, m, v out)
    adam-off        jd_optimizer_step, no option        36 B  (the same kernel through the other entry)
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
--against PATH (repeatable): other builds of the library, e.g. a parent commit's (make -C jolideco_amd/csrc VARIANT=parent
there, the .so copied beside the in-tree one) and a second copy of it under another name -- parent against parent is the
spread.  jd_adam_step, jd_sgd_step, jd_adam_step_addends with 2 addends and jd_optimizer_step with amsgrad of every library:
first one step on equal seeded images and `torch.equal` of what the plain entries wrote, then all of them timed alternating.
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


AGAINST_ENTRIES = ("jd_adam_step", "jd_sgd_step", "jd_adam_step_addends", "jd_optimizer_step")
AGAINST_PLAIN = ("adam", "sgd", "adam-addends2")  # (held to the other libraries' bits and time; adam-amsgrad is only reported)


def load_library(path):
    """The step entries of another build of the library (a parent commit's), with the argument types of `_hip.EXPORTS`."""
    from jolideco_amd import _hip

    handle = ctypes.CDLL(str(Path(path).resolve()))
    for name in AGAINST_ENTRIES:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _hip.EXPORTS[name]
    return handle


def against_variants(n, device, libs, seed=1):
    """{entry: {library: (call, images)}} for jd_adam_step, jd_sgd_step, jd_adam_step_addends with 2 addends and
    jd_optimizer_step with amsgrad, of every library in `libs` on images of its own drawn from the SAME seed per entry."""
    from jolideco_amd import _hip
    from jolideco_amd._hip import check, ptr, ptr_array, stream_ptr
    from jolideco_amd.ops import adam_bias_terms

    new = lambda a: torch.from_numpy(a.astype(np.float32)).to(device)  # noqa: E731
    lr, beta1, beta2, eps = 1e-3, 0.9, 0.999, 1e-8
    step_size, bias2_sqrt = adam_bias_terms(10, lr, beta1, beta2)
    adam_terms = (step_size, beta1, beta2, 1 - beta1, 1 - beta2, bias2_sqrt, eps)
    stream = stream_ptr(device)
    amsgrad = _hip.OptimizerOptions(kind=_hip.OPTIMIZER_ADAM, step_size=step_size, beta1=beta1, beta2=beta2, one_minus_beta1=1 - beta1,
                                    one_minus_beta2=1 - beta2, bias2_sqrt=bias2_sqrt, eps=eps, lr=lr, amsgrad=1)

    def images(entry, entry_seed):
        rs = np.random.RandomState(entry_seed)
        theta = rs.normal(size=n)
        im = {"theta": new(theta), "flux_in": new(np.exp(theta)), "flux_out": new(np.zeros(n)), "grad": new(rs.normal(size=n))}
        if entry != "sgd":
            im["exp_avg"], im["exp_avg_sq"] = new(0.1 * rs.normal(size=n)), new(rs.uniform(size=n) ** 2)
        if entry == "adam-addends2":
            im["addends"] = [new(rs.normal(size=n)), new(rs.normal(size=n))]
            im["addend_array"] = ptr_array(im["addends"] + [None, None])  # (JD_ADDEND_MAX = 4 entries)
        if entry == "adam-amsgrad":
            im["max_exp_avg_sq"] = new(rs.uniform(size=n) ** 2)
        return im

    def call(entry, lib, im):
        head = (ptr(im["theta"]), ptr(im["flux_in"]), ptr(im["flux_out"]), ptr(im["grad"]))
        if entry == "sgd":
            return lambda: check(lib.jd_sgd_step(*head, None, n, lr, 0, 1, stream))
        moments = (ptr(im["exp_avg"]), ptr(im["exp_avg_sq"]))
        if entry == "adam":
            return lambda: check(lib.jd_adam_step(*head, *moments, None, n, *adam_terms, 0, 1, None, stream))
        if entry == "adam-addends2":
            return lambda: check(lib.jd_adam_step_addends(*head, *moments, None, n, *adam_terms, 0, 1, None, im["addend_array"], stream))
        return lambda: check(lib.jd_optimizer_step(*head, *moments, ptr(im["max_exp_avg_sq"]), None, None, n, ctypes.byref(amsgrad), 0, 1,
                                                   None, stream))

    out = {}
    for k, entry in enumerate(AGAINST_PLAIN + ("adam-amsgrad",)):
        out[entry] = {}
        for name, lib in libs.items():
            im = images(entry, seed + k)
            out[entry][name] = (call(entry, lib, im), im)
    return out


def run_against(paths, n, steps, warmup, repeats, device):
    """The in-tree library ("child") against the libraries of `paths`: one step of every plain entry on equal images and
    `torch.equal` of what it wrote, then the timing of `time_steps` over every (entry, library), alternating.  Per plain
    entry: whether the child's median lies inside or below the band of round medians the other libraries span together."""
    from jolideco_amd import _hip

    libs = {"child": _hip.lib()}
    libs.update({Path(p).stem.replace("libjolideco_hip_", ""): load_library(p) for p in paths})
    variants = against_variants(n, device, libs)
    bits = {}
    for entry in AGAINST_PLAIN:
        for call, _ in variants[entry].values():
            call()
        torch.cuda.synchronize(device)
        child = variants[entry]["child"][1]
        bits[entry] = {name: {key: bool(torch.equal(im[key], child[key])) for key in ("theta", "flux_out", "exp_avg", "exp_avg_sq") if key in im}
                       for name, (_, im) in variants[entry].items() if name != "child"}
    calls = {f"{entry}@{name}": call for entry, by_lib in variants.items() for name, (call, _) in by_lib.items()}
    medians, spread = time_steps(calls, steps, warmup, repeats, device)
    out = {"libraries": list(libs), "bits_equal": bits, "steps_us": medians, "steps_us_min_max": spread, "plain_entries": {}}
    for entry in AGAINST_PLAIN:
        others = [spread[f"{entry}@{name}"] for name in libs if name != "child"]
        band = (min(lo for lo, _ in others), max(hi for _, hi in others))
        child = medians[f"{entry}@child"]
        out["plain_entries"][entry] = {"child_us": child, "band_us": band, "inside_or_below": child <= band[1]}
    return out


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
    ap.add_argument("--against", action="append", default=[], metavar="PATH",
                    help="another build of the library (repeatable): its step entries are held to the in-tree build's bits and time")
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
    if args.against:
        result["against"] = run_against(args.against, n, args.steps, args.warmup, args.repeats, device)
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

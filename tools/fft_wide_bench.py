"""The native FFT convolution against the rocFFT plan on images beyond 4608-point rows / 2304-point columns -- the sizes that
ran on rocFFT until the "generic-huge" row kernels and the four-wave column kernel (csrc/fftnative.hip).

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 500 python tools/fft_wide_bench.py [--out FILE.json] [--only NAME]

Per geometry two calls, each on a native plan and on the rocFFT plan of the SAME build (option JD_FFT_NATIVE=0 while the plan
is created -- what these sizes ran before):
    fwd    ConvPlan.conv_same with an exposure image: rows, columns, rows^-1 (three launches on the native plan)
    step   ConvPlan.npred_poisson_fwd_bwd, one dataset, gradient accumulated: the five-launch likelihood step
Boards differ by several percent and drift with temperature, so the two plans run ALTERNATING in one process after a
warm-up; each call is bracketed by device events, and the median over --repeats rounds of --steps calls is reported with the
smallest and largest round median.  The work arrays of these sizes (0.3 to 0.7 GB) do not stay in the 256 MiB last-level cache
from launch to launch.

Yardstick: the bytes the native launches move between HBM and the CUs per image pixel (`native_bytes`: images, spectrum rows,
the kept rows of the column pass, the kernel spectrum), and the fraction of 8 TB/s that is at the measured time."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

GEOMETRIES = {
    "8192x8192-k17": ((8192, 8192), 17),
    "8192x8192-k65": ((8192, 8192), 65),
    "4096x8192-k17": ((4096, 8192), 17),
    "6000x6000-k17": ((6000, 6000), 17),
    "8192x512-k17": ((8192, 512), 17),
}
HBM_BYTES_PER_S = 8e12


def native_bytes(H, W, k, Nx, Ny, step):
    """HBM bytes of the native launches: rows (image + exposure in, Hh spectrum rows out), columns (those in, the kernel
    spectrum in, the Hh + k - 1 kept rows out), rows^-1 (those in, image out).  A step: the forward's three launches with the
    middle one reading background and counts and writing the row spectra of g, the adjoint's columns, and rows^-1 reading the
    exposure and updating the gradient image."""
    Hh = (H + 1) // 2
    image, spec, kept, khat = 4 * H * W, 8 * Hh * Nx, 8 * (Hh + k - 1) * Nx, 8 * Nx * Ny
    forward = 2 * image + spec + spec + khat + kept + kept + image
    if not step:
        return forward
    return (2 * image + spec) + (spec + khat + kept) + (kept + 2 * image + spec) + (spec + khat + kept) + (kept + 3 * image)


def make_case(shape, k, native, device):
    from jolideco_amd import _hip
    from jolideco_amd.ops import ConvPlan, stirling_mean

    H, W = shape
    rs = np.random.RandomState(H + W + k)
    psf = rs.uniform(size=(k, k)) ** 3 + 0.2
    psf = (psf / psf.sum()).astype(np.float32)
    previous = _hip.get_option("JD_FFT_NATIVE")
    _hip.set_option("JD_FFT_NATIVE", 1 if native else 0)
    try:
        plan = ConvPlan(H, W, k, k, device, method="fft")
    finally:
        _hip.set_option("JD_FFT_NATIVE", previous)
    assert plan.native_fft == native, (shape, k, native)
    new = lambda a: torch.from_numpy(a.astype(np.float32)).to(device)  # noqa: E731
    counts = rs.poisson(6.0, size=shape)
    t = {"flux": new(0.5 + rs.gamma(2.0, size=shape)), "exposure": new(rs.uniform(0.5, 1.5, size=shape)),
         "background": new(rs.uniform(0.5, 1.0, size=shape)), "counts": new(counts), "grad": torch.zeros(shape, device=device),
         "loss": torch.zeros(1, device=device)}
    t["khat"] = plan.psf_spectrum(new(psf))
    stirling = stirling_mean(counts)

    def fwd():
        return plan.conv_same(t["flux"], t["exposure"], t["khat"])

    def step():
        plan.npred_poisson_fwd_bwd([t["flux"]], [t["exposure"]], [t["khat"]], t["background"], t["counts"], stirling, t["loss"],
                                   grads=[t["grad"]], accumulate=True, grad_scale=1e-3)

    return plan, t, {"fwd": fwd, "step": step}


def time_calls(calls, steps, warmup, repeats, device):
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize(device)
    rounds = {name: [] for name in calls}
    for _ in range(repeats):
        pairs = {name: [] for name in calls}
        for _ in range(steps):
            for name, call in calls.items():  # (alternating: a drift of the board hits both plans alike)
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                call()
                end.record()
                pairs[name].append((start, end))
        torch.cuda.synchronize(device)
        for name, events in pairs.items():
            rounds[name].append(float(np.median([s.elapsed_time(e) for s, e in events])) * 1e3)
    return {name: {"us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for name, v in rounds.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", action="append", default=[], choices=sorted(GEOMETRIES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import _hip

    device = torch.device("cuda:0")
    result = {"clock_mhz": _hip.clock_probe(device=device), "geometries": {}}
    for name in args.only or GEOMETRIES:
        shape, k = GEOMETRIES[name]
        cases = {kind: make_case(shape, k, kind == "native", device) for kind in ("native", "rocfft")}
        route = cases["native"][0].step_route(1, 1)
        calls = {f"{call}@{kind}": fn for kind, (_, _, fns) in cases.items() for call, fn in fns.items()}
        times = time_calls(calls, args.steps, args.warmup, args.repeats, device)
        entry = {"Nx": route["Nx"], "Ny": route["Ny"], "rows": route["rows_fwd"], "times": times}
        for call in ("fwd", "step"):
            moved = native_bytes(*shape, k, route["Nx"], route["Ny"], call == "step")
            us = times[f"{call}@native"]["us"]
            entry[call] = {"native_us": us, "rocfft_us": times[f"{call}@rocfft"]["us"], "speedup": times[f"{call}@rocfft"]["us"] / us,
                           "bytes_per_pixel": moved / (shape[0] * shape[1]), "fraction_of_8_tb_s": moved / (us * 1e-6) / HBM_BYTES_PER_S}
        result["geometries"][name] = entry
        print(name, json.dumps(entry), flush=True)
        for plan, tensors, _ in cases.values():
            torch.cuda.synchronize(device)
            plan.close()
            tensors.clear()
        del cases, calls
        torch.cuda.empty_cache()
    result["clock_mhz_after"] = _hip.clock_probe(device=device)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

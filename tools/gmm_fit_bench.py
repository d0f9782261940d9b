"""Time per EM step of `GaussianMixtureModel.fit` (csrc/gmm_fit.hip), beside the kernel's flop and byte counts.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 600 python tools/gmm_fit_bench.py [--out FILE.json]

Cases: n = 2^18 and 2^20 patches with K = 128, D = 64, and with K = 200, D = 256.  The patches are mean-free draws of
`data.synthetic_gmm`-like clusters, the start is the random start of `fit`; every case runs --warmup steps and then times
--steps single steps.  A step is timed in two parts: the device part (upload of the K D^2 factors, the two launches, the
copy of the K (D^2 + D + 1) + 1 sums to the host: wall clock around `ops.GmmFitHandle.step`, which synchronises) and the
host part (Cholesky factors and the float64 M-step).  The median over the steps is reported.

Counts per step (printed with the times):
  flops   n K x [2 passes x 2 x 256 NJ (NJ + 1) / 2 (whitening on the f32 MFMA, NJ = D / 16, zero blocks skipped)
                 + 2 D^2 (second moments on the f64 MFMA)]
  bytes   what the kernel asks of L2: n D 4 x K x (1 + D / 64) (the patches, staged once per component in the first
          pass and once per component and 64-row panel in the second), the factors K D (D + 16) / 2 x 4 per 64-patch tile
          and pass, and one read-add-write of the blocks' K (D^2 + D + 1) doubles per 2048-patch chunk.
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

CASES = [(64, 128, 2**18), (64, 128, 2**20), (256, 200, 2**18), (256, 200, 2**20)]  # (D, K, n)


def counts(D, K, n):
    nj = D // 16
    flops = n * K * (2 * 2 * 256 * nj * (nj + 1) // 2 + 2 * D * D)
    tiles = -(-n // 64)
    bytes_x = n * D * 4 * K * (1 + D // 64)
    bytes_p = tiles * 2 * K * D * (D + 16) // 2 * 4
    bytes_partials = -(-n // 2048) * K * (D * D + D + 1) * 16
    return flops, bytes_x + bytes_p + bytes_partials


def patches(D, n, device, seed=0):
    gen = torch.Generator(device=device).manual_seed(seed)
    centres = 2.0 * torch.randn(6, D, device=device, generator=gen)
    scales = torch.linspace(0.3, 1.5, D, device=device)
    label = torch.randint(0, 6, (n,), device=device, generator=gen)
    x = centres[label] + torch.randn(n, D, device=device, generator=gen) * scales
    return (x - x.mean(dim=1, keepdim=True)).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", type=int, nargs="+", default=list(range(len(CASES))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from jolideco_amd import _hip, ops
    from jolideco_amd.priors.patches import gmm as gmm_module

    device = torch.device("cuda:0")
    results = []
    for index in args.cases:
        D, K, n = CASES[index]
        x = patches(D, n, device)
        means, covariances, weights = gmm_module.random_start(x, K)
        handle = gmm_module._fit_handle(ops.GmmFitHandle, device, D, K)
        device_s, host_s, bounds = [], [], []
        real_step = handle.step

        def timed_step(*a):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real_step(*a)
            device_s.append(time.perf_counter() - t0)
            return out

        handle.step = timed_step
        for _ in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            means, covariances, weights, bound, _ = gmm_module.em_step(handle, x, means, covariances, weights, 1e-6)
            host_s.append(time.perf_counter() - t0 - device_s[-1])
            bounds.append(bound)
        handle.step = real_step
        dev, host = float(np.median(device_s[args.warmup:])), float(np.median(host_s[args.warmup:]))
        flops, nbytes = counts(D, K, n)
        row = {"D": D, "K": K, "n": n, "device_ms": 1e3 * dev, "host_ms": 1e3 * host, "gflop": flops / 1e9, "gbyte": nbytes / 1e9,
               "tflops": flops / dev / 1e12, "tbytes_per_s": nbytes / dev / 1e12, "lower_bounds": bounds,
               "clock_mhz": _hip.clock_probe(device=device)}
        print(json.dumps(row), flush=True)
        results.append(row)
        del x
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()

"""Time of one Lloyd step (csrc/kmeans.hip) beside one EM step (csrc/gmm_fit.hip) at the same shape IN THE SAME RUN, and
the EM steps to convergence of `GaussianMixtureModel.fit_images` from the k-means start and from the random-patches start.

Run by hand on the GPU box, one process, under a timeout:
    timeout -k 10 900 python tools/kmeans_bench.py [--out FILE.json]

Part 1, shapes (n, K, D) = (10^6, 128, 64) and (2.5 10^5, 200, 256): mean-free draws of a few broad clusters (the data of
tools/gmm_fit_bench.py), the centres K of the patches, the EM parameters the random start of `fit`.  Both steps are timed
the same way: device events around the library call alone (`jd_kmeans_step`: three launches; `jd_gmm_fit_step`: two), no
upload and no copy of the sums inside the window; --warmup calls, then --repeats timed regions of --calls calls each, the
median region reported per call, alternating the two kernels region by region.  Every line carries the shader clock
measured right after its regions (`_hip.clock_probe`).  The acceptance condition -- a Lloyd step takes no longer than the
EM step of the shape -- is evaluated and printed; the exit status is 1 where it fails.

Counts per Lloyd step (printed with the times):
  flops   2 n K D on the f32 MFMA (assignment, centre tiles padded to 16) + 2 n D 16 ceil(K / 16) on the f64 MFMA (one-hot
          sums: every patch meets every centre tile of its block) + 3 n D float64 VALU (inertia)
  bytes   from HBM: the patches once for the assignment and once per group of KG centre tiles for the sums (G =
          ceil(ceil(K / 16) / KG) groups, KG = 8 at D = 64 and 4 at D = 256: 1 and 4 at the two shapes), (1 + G) n D 4; the
          labels read and written by the assignment and read by every group, n (8 + 4 G); the blocks' partial sums written
          and read again by the reduce launch, 2 x blocks x (K (D + 1) + 3) x 8 with blocks = min(ceil(n / 512), 2 CUs);
          asked of L2: the centres K D 4 once per tile of 64 or 128 patches.
Part 2, for each scene of --scenes ("points": 40 point sources and 6 smooth blobs on a background of 2 counts; "smooth": the
blobs alone on a background of 20) and each K of --components: --images synthetic images with Poisson noise, 8 x 8 patches at
stride 2, subtract-mean norm, tol = 1e-3: the EM steps until convergence, the first and the final lower bound and the wall
time of the whole fit from both starts; a fit that ends in a starved component is recorded with its message.  Recorded,
not gated.
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

SHAPES = [(10**6, 128, 64), (250000, 200, 256)]  # (n, K, D)


def lloyd_counts(n, K, D, n_cu):
    kt = -(-K // 16)
    tile, kg = (128, 8) if D == 64 else (64, 4)
    groups = -(-kt // kg)
    blocks = min(-(-n // 512), 2 * n_cu)
    flops = 2 * n * 16 * kt * D + 2 * n * D * 16 * kt + 3 * n * D
    hbm = (1 + groups) * n * D * 4 + n * (8 + 4 * groups) + 2 * blocks * (K * (D + 1) + 3) * 8
    l2 = -(-n // tile) * K * D * 4
    return flops, hbm, l2


def patches(D, n, device, seed=0):
    gen = torch.Generator(device=device).manual_seed(seed)
    centres = 2.0 * torch.randn(6, D, device=device, generator=gen)
    scales = torch.linspace(0.3, 1.5, D, device=device)
    label = torch.randint(0, 6, (n,), device=device, generator=gen)
    x = centres[label] + torch.randn(n, D, device=device, generator=gen) * scales
    return (x - x.mean(dim=1, keepdim=True)).contiguous()


def region_ms(call, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def step_times(args, device):
    from jolideco_amd import _hip, ops
    from jolideco_amd.priors.patches import gmm as gmm_module
    from jolideco_amd.utils.numpy import compute_precision_cholesky

    rows = []
    for n, K, D in SHAPES:
        x = patches(D, n, device)
        pick = torch.from_numpy(np.sort(np.random.RandomState(0).choice(n, K, replace=False))).to(device)
        centres = x[pick].contiguous()
        labels = torch.full((n,), -1, dtype=torch.int32, device=device)
        km = ops.KMeansHandle(D, K, device)
        means, covariances, weights = gmm_module.random_start(x, K)
        prec = compute_precision_cholesky(covariances).astype(np.float32)
        const = np.log(weights) + np.log(np.diagonal(prec, axis1=1, axis2=2).astype(np.float64)).sum(axis=1) - 0.5 * D * np.log(2 * np.pi)
        em = ops.GmmFitHandle(D, K, device)
        em_args = [gmm_module._upload(a, device) for a in (means, prec, const)]
        lib, stream = _hip.lib(), _hip.stream_ptr(device)

        def lloyd():
            km.launch(x, centres, labels)

        def em_step():
            _hip.check(lib.jd_gmm_fit_step(em._handle, _hip.ptr(x), n, *(_hip.ptr(a) for a in em_args),
                                           _hip.ptr(em.sums), stream))

        for _ in range(args.warmup):
            lloyd()
            em_step()
        torch.cuda.synchronize()
        t_lloyd, t_em = [], []
        for _ in range(args.repeats):  # alternating, region by region
            t_lloyd.append(region_ms(lloyd, args.calls))
            t_em.append(region_ms(em_step, 1))
        clock = _hip.clock_probe(device=device)
        flops, hbm, l2 = lloyd_counts(n, K, D, torch.cuda.get_device_properties(device).multi_processor_count)
        ms_lloyd, ms_em = float(np.median(t_lloyd)), float(np.median(t_em))
        sums = km.sums.cpu().numpy()
        row = {"part": "step", "n": n, "K": K, "D": D, "lloyd_ms": ms_lloyd, "lloyd_ms_min_max": [min(t_lloyd), max(t_lloyd)],
               "em_ms": ms_em, "em_ms_min_max": [min(t_em), max(t_em)], "em_over_lloyd": ms_em / ms_lloyd,
               "lloyd_gflop": flops / 1e9, "lloyd_tflops": flops / ms_lloyd / 1e9, "lloyd_hbm_gb": hbm / 1e9,
               "lloyd_hbm_tb_per_s": hbm / ms_lloyd / 1e9, "lloyd_l2_gb": l2 / 1e9, "inertia": float(sums[-3]),
               "empty_clusters": int((sums[:K] == 0).sum()), "clock_mhz": clock, "lloyd_not_slower": ms_lloyd <= ms_em}
        print(json.dumps(row), flush=True)
        rows.append(row)
        km.close()
        em.close()
        del x, labels
    return rows


SCENES = {"points": (2.0, ((1.5, 400.0, 40), (12.0, 60.0, 6))), "smooth": (20.0, ((12.0, 60.0, 6),))}


def synthetic_images(count, size, device, scene="points", seed=0):
    gen = torch.Generator(device=device).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size, device=device, dtype=torch.float32), torch.arange(size, device=device, dtype=torch.float32),
                            indexing="ij")
    images = []
    for _ in range(count):
        background, sources = SCENES[scene]
        flux = torch.full((size, size), background, device=device)
        for width, amplitude, number in sources:
            pos = torch.rand(number, 2, device=device, generator=gen) * size
            amp = amplitude * torch.rand(number, device=device, generator=gen)
            for (py, px), a in zip(pos.tolist(), amp.tolist()):
                flux += a * torch.exp(-((yy - py) ** 2 + (xx - px) ** 2) / (2 * width * width))
        images.append(torch.poisson(flux, generator=gen))
    return images


def convergence(args, device):
    from jolideco_amd import _hip
    from jolideco_amd.priors.patches import GaussianMixtureModel

    rows = []
    for scene, components, start in ((c, k, s) for c in args.scenes for k in args.components for s in ("kmeans", "random-patches")):
        images = synthetic_images(args.images, args.size, device, scene)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row = {"part": "fit", "scene": scene, "start": start, "K": components, "images": args.images, "size": args.size}
        try:
            model = GaussianMixtureModel.fit_images(images, stride=2, n_components=components, n_iter=args.max_em, tol=1e-3,
                                                    init_params=start)
            info = model.fit_info
            row.update(em_steps=info["n_iter"], converged=info["converged"], lower_bound=info["lower_bounds"][-1],
                       first_lower_bound=info["lower_bounds"][0], smallest_weight=float(info["weights"].min()))
            if "kmeans" in info:
                row.update(lloyd_steps=info["kmeans"]["n_iter"], lloyd_converged=info["kmeans"]["converged"],
                           smallest_cluster=int(info["kmeans"]["counts"].min()))
        except ValueError as exc:  # a starved component ends a fit: recorded
            row.update(error=str(exc)[:200])
        torch.cuda.synchronize()
        row.update(wall_s=time.perf_counter() - t0, clock_mhz=_hip.clock_probe(device=device))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="Lloyd steps per timed region (an EM region is one step)")
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--components", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    ap.add_argument("--max-em", type=int, default=300)
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs a HIP device: nothing is measured without one")
    device = torch.device("cuda:0")
    rows = [] if args.skip_steps else step_times(args, device)
    if not args.skip_fit:
        rows += convergence(args, device)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1))
    return 0 if all(r.get("lloyd_not_slower", True) for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())

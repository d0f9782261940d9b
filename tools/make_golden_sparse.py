"""Generate tests/golden/sparse_component.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_sparse.py

The sparse point-source flux component.  From the reference's `SparseSpatialFluxComponent`: (a) its own test case (3 sources
on 25 x 25) and (b) a collision case on 12 x 16 (two sources in one pixel cell, two that share one pixel, one on exactly
integer coordinates, one half a pixel beyond the last column, one wholly outside) -- the rendered image and the autograd
gradients of sum(R * image) for a seeded random R; (c) a 6-epoch sequential fit of a 32 x 32 scene (two observations) with a
diffuse `SpatialFluxComponent` and 3 sources started about 0.7 pixels from the true positions, one of them on an exactly
integer x.  While generating, the oracle and the fit harness of tests/sparse_cases.py are asserted to reproduce the reference
-- they are what the GPU tests compare against.  The fixture holds data only.
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("make_golden", REPO / "oracle" / "refload" / "make_golden.py")
mg = importlib.util.module_from_spec(spec)
sys.modules["make_golden"] = mg
spec.loader.exec_module(mg)  # runs load_reference()
sys.path.insert(0, str(REPO / "tests"))

from jolideco.core import MAPDeconvolver  # noqa: E402
from jolideco.models import FluxComponents, SparseSpatialFluxComponent, SpatialFluxComponent  # noqa: E402

import sparse_cases as cases  # noqa: E402


def ulps(a, b):
    """Largest difference of two float32 arrays in units in the last place of the larger magnitude."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    spacing = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / spacing)) if a.size else 0.0


def render_case(tag, sources, shape, out):
    flux, x_pos, y_pos = sources
    upstream = cases.upstream(shape)
    for use_log_flux in (True, False):
        component = SparseSpatialFluxComponent.from_numpy(flux=flux, x_pos=x_pos, y_pos=y_pos, shape=shape,
                                                          use_log_flux=use_log_flux)
        image = component.flux
        (image[0, 0] * torch.from_numpy(upstream)).sum().backward()
        grads = [p.grad.numpy() for p in (component._flux, component.x_pos, component.y_pos)]
        param = cases.parameter(flux, use_log_flux)
        assert np.array_equal(param, component._flux.detach().numpy())
        image_o, grads_o = cases.oracle(param, x_pos, y_pos, shape, use_log_flux, upstream, dtype=np.float32)
        image_r = image.detach().numpy()[0, 0]
        if not np.array_equal(image_o, image_r):
            worst = ulps(image_o, image_r)
            assert worst <= 1.0, (tag, worst)
            print(f"sparse {tag}: torch's reduction order differs, the image is held to 1 ulp (worst {worst:.2f})")
        for g_o, g_r in zip(grads_o, grads):
            assert np.array_equal(g_o.astype(np.float32), g_r), (tag, use_log_flux)
        image64, grads64 = cases.oracle(param, x_pos, y_pos, shape, use_log_flux, upstream, dtype=np.float64)
        assert cases.rel_linf(image_r, image64) < 1e-6
        assert all(cases.rel_linf(g, g64) < 1e-5 for g, g64 in zip(grads, grads64))
        key = f"{tag}/{'log' if use_log_flux else 'linear'}"
        out[f"{key}/image"] = image_r
        for name, g in zip(("grad_param", "grad_x", "grad_y"), grads):
            out[f"{key}/{name}"] = g
        print("sparse", key, "ok", float(image_r.sum()))
    out[f"{tag}/flux"], out[f"{tag}/x_pos"], out[f"{tag}/y_pos"] = flux, x_pos, y_pos
    out[f"{tag}/shape"] = np.array(shape)


def main():
    torch.manual_seed(0)
    out = {}
    render_case("a", cases.case_a(), cases.CASE_A_SHAPE, out)
    render_case("b", cases.case_b(), cases.CASE_B_SHAPE, out)
    # the axes: x_pos runs along the rows
    probe = SparseSpatialFluxComponent.from_numpy(flux=1.0, x_pos=2.0, y_pos=7.25, shape=(5, 10)).flux.detach().numpy()[0, 0]
    assert np.argwhere(probe > 0).tolist() == [[2, 7], [2, 8]]

    # (c) the fit
    datasets, truth = cases.fit_scene(scene=mg.scene, asym_psf=mg.asym_psf)
    flux_init, sources = cases.fit_start(truth)
    assert float(sources[1][-1]) == round(float(sources[1][-1])), "the last source starts on an integer x"
    components = FluxComponents()
    components["diffuse"] = SpatialFluxComponent.from_numpy(flux=flux_init)
    components["points"] = SparseSpatialFluxComponent.from_numpy(flux=sources[0], x_pos=sources[1], y_pos=sources[2],
                                                                 shape=cases.FIT_SHAPE)
    res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False).run(datasets=datasets, components=components)
    points = res.components["points"]
    run = cases.fit_harness(datasets, flux_init, sources, cases.FIT_EPOCHS, record_first_grads=True)
    assert np.array_equal(run["diffuse"], res.components["diffuse"].flux_upsampled_numpy)
    assert np.array_equal(run["x_pos"], points.x_pos_numpy) and np.array_equal(run["y_pos"], points.y_pos_numpy)
    assert np.array_equal(run["flux"], points.to_dict()["flux"])
    assert [row["total"] for row in run["trace"]] == [float(v) for v in res.trace_loss["total"]]
    assert points.x_pos_numpy[-1] == sources[1][-1], "a source on an integer x never moves along x"
    # Adam's first step is lr * sign(g): no position gradient may be rounding noise
    g_x, g_y = run["first_grads"][1], run["first_grads"][2]
    largest = max(np.abs(g_x).max(), np.abs(g_y).max())
    for g in np.concatenate([g_x, g_y]):
        assert g == 0.0 or abs(g) >= 1e-3 * largest, (g_x, g_y)
    assert g_x[-1] == 0.0 and np.count_nonzero(np.concatenate([g_x, g_y])) == 2 * len(g_x) - 1
    moved = np.hypot(points.x_pos_numpy - sources[1], points.y_pos_numpy - sources[2])
    print("sparse fit ok: moved", moved, "first gradients", g_x, g_y, "total", res.trace_loss[-1]["total"])
    out.update({f"fit/{k}": v for k, v in mg.pack_datasets(datasets).items()})
    out.update({"fit/flux_init": flux_init, "fit/start/flux": sources[0], "fit/start/x_pos": sources[1],
                "fit/start/y_pos": sources[2], "fit/truth": np.array(truth, dtype=np.float64),
                "fit/diffuse": res.components["diffuse"].flux_upsampled_numpy, "fit/image": points.flux_numpy,
                "fit/flux": points.to_dict()["flux"], "fit/x_pos": points.x_pos_numpy, "fit/y_pos": points.y_pos_numpy})
    out.update({f"fit/{k}": v for k, v in mg.trace_to_arrays(res.trace_loss).items()})

    path = REPO / "tests" / "golden" / "sparse_component.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

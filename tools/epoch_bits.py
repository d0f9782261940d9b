"""One sha256 per fit over everything a fit produces -- fluxes, thetas, the scalars of every epoch, calibration values (for
a sparse component: its source vectors): the six fits of tests/test_gpu_graph.py with host scalars, device scalars and
captured epochs, a fit with a sparse component, an SGD fit, and the sessions of tests/test_gpu_epoch_body.py.  Run it with
two versions of the Python package against ONE built library (JOLIDECO_HIP_LIBRARY) and compare the outputs: a change to
the host side of an epoch that changes no bit prints the same lines.

    python tools/epoch_bits.py [directory to import jolideco_amd from]"""
import hashlib
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(sys.argv[1]).resolve() if len(sys.argv) > 1 else REPO))
sys.path.insert(1, str(REPO))
sys.path.insert(2, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


class _Environment:
    """`monkeypatch.setenv` for `test_gpu_graph._fit`, outside pytest."""

    @staticmethod
    def setenv(key, value):
        os.environ[key] = value


def main():
    import jolideco_amd
    import sparse_cases
    import test_gpu_epoch_body as body
    import test_gpu_graph as graph
    from jolideco_amd.distributed import DistContext

    print("jolideco_amd from", Path(jolideco_amd.__file__).parent, file=sys.stderr)
    assert Path(jolideco_amd.__file__).resolve().is_relative_to(Path(sys.path[0]))
    for case in sorted(graph.CASES):
        build, fit_mode = graph.CASES[case]
        for mode in ("host", "device", "graph"):
            fluxes, rows, cal, n_graphs, _ = graph._fit(_Environment, mode, build, 9, fit_mode)
            print(f"{case}/{mode}: {digest(fluxes + [rows] + cal)} graphs={n_graphs}", flush=True)
    for key in ("JOLIDECO_STEP_SCALARS", "JOLIDECO_GRAPH"):
        os.environ.pop(key, None)

    # a sparse component beside a diffuse one (by value always)
    for fit_mode in ("joint", "sequential"):
        datasets, flux_init = _sparse_scene()
        session = jolideco_amd.MAPDeconvolver(n_epochs=6, display_progress=False, device=body.DEV, fit_mode=fit_mode).session(
            datasets, components=_sparse_components(jolideco_amd, sparse_cases, flux_init))
        rows = []
        for _ in range(6):
            session.epoch()
            rows.append(session.scalars.clone())
        torch.cuda.synchronize()
        points = session.components["points"]
        arrays = [st.flux_cur.cpu().numpy() for st in session.states] + [torch.stack(rows).cpu().numpy()]
        arrays += [p.detach().cpu().numpy() for p in (points._flux, points.x_pos, points.y_pos)]
        print(f"sparse-{fit_mode}: {digest(arrays)}", flush=True)

    sharded = dict(rank=0, world_size=1, dry_run=True, force_collectives=True)
    sessions = {"sgd": dict(optimizer_type="sgd"), "hook": dict(hook=True), "hook-uniform": dict(hook=True, uniform=True),
                "validation": dict(validation=True), "sharded": dict(dist=sharded), "sharded-uniform": dict(dist=sharded, uniform=True)}
    for name, kwargs in sessions.items():
        for fit_mode in ("joint", "sequential"):
            if "dist" in kwargs:
                kwargs = dict(kwargs, dist=DistContext(**sharded))  # (a context of its own for every session)
            result = body.fit(fit_mode, **kwargs)
            print(f"{name}-{fit_mode}: {digest(result['images'] + [result['scalars']])}", flush=True)


def _sparse_scene():
    from conftest import unpack_datasets

    g = dict(np.load(REPO / "tests" / "golden" / "sparse_component.npz"))
    return unpack_datasets(g, prefix="fit/data/"), g["fit/flux_init"]


def _sparse_components(jd, cases, flux_init):
    g = dict(np.load(REPO / "tests" / "golden" / "sparse_component.npz"))
    comps = jd.FluxComponents()
    comps["diffuse"] = jd.SpatialFluxComponent.from_numpy(flux=flux_init)
    comps["points"] = jd.SparseSpatialFluxComponent.from_numpy(
        flux=g["fit/start/flux"], x_pos=g["fit/start/x_pos"], y_pos=g["fit/start/y_pos"], shape=cases.FIT_SHAPE)
    return comps


if __name__ == "__main__":
    main()

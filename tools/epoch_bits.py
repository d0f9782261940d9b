"""One sha256 per fit over everything a fit produces -- fluxes, thetas, the scalars of every epoch, calibration values (for
a sparse component: its source vectors): the six fits of tests/test_gpu_graph.py with host scalars, device scalars and
captured epochs, a fit with a sparse component, an SGD fit, and the sessions of tests/test_gpu_epoch_body.py.  Run it with
two versions of the Python package against ONE built library (JOLIDECO_HIP_LIBRARY) and compare the outputs: a change to
the host side of an epoch that changes no bit prints the same lines.

Section "patches": one sha256 per low-level `GmmHandle.prior_fwd_bwd` call over the value, the gradient image and the
arg-max -- every case of tests/gmm_subpix_cases.py and tests/gmm_jitter_cases.py (both patch sizes) as the plain pass, as the
staged pass with its draws by value / on the host, and with them in device memory; max and logsumexp (the latter with the
screen off, JD_GMM_LSE_SCREEN=0, and forced, =2: by default the host's timing picks the route), identity and asinh image
norm, both patch norms; the gradient accumulated with coefficient 0.75 into a non-zero image, no gradient, and the value
accumulated -- and the two six-epoch fits of those modules.  This section also compares two LIBRARIES.  "patches-brief"
makes the same calls and prints, for every case and route (max, logsumexp with the screen off, with it forced), one sha256
over the 36 lines "patches" prints for it -- the listing to keep; "patches" says which call differs.

    python tools/epoch_bits.py [directory to import jolideco_amd from] [fits | patches | patches-brief ...]"""
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

    print("jolideco_amd from", Path(jolideco_amd.__file__).parent, file=sys.stderr)
    assert Path(jolideco_amd.__file__).resolve().is_relative_to(Path(sys.path[0]))
    sections = sys.argv[2:] or ["fits", "patches"]
    if "fits" in sections:
        fit_bits(jolideco_amd)
    if "patches" in sections or "patches-brief" in sections:
        patch_prior_bits(jolideco_amd, brief="patches" not in sections)


def fit_bits(jolideco_amd):
    import sparse_cases
    import test_gpu_epoch_body as body
    import test_gpu_graph as graph
    from jolideco_amd.distributed import DistContext

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


DEV = "cuda:0"


def _prior_call_digest(handle, flux, stride, roll, setup, marginalize, **kwargs):
    """One call.  ``setup``: "grad" -- the gradient accumulated with coefficient 0.75 into a non-zero image | "forward" -- no
    gradient | "value" -- the value accumulated onto 2.5 (gradient with coefficient 1 into zeros)."""
    value = torch.full((1,), 2.5 if setup == "value" else float("nan"), device=DEV)
    grad = {"grad": lambda: 0.01 * flux, "forward": lambda: None, "value": lambda: torch.zeros_like(flux)}[setup]()
    argmax = None if marginalize else torch.full((flux.numel(),), -7, dtype=torch.int32, device=DEV)  # (more than the patches)
    handle.prior_fwd_bwd(flux, stride, roll, value, 1.0, grad=grad, grad_coef=0.75 if setup == "grad" else 1.0,
                         marginalize=marginalize, argmax_out=argmax, accumulate_value=setup == "value", **kwargs)
    torch.cuda.synchronize()
    return digest([t.cpu().numpy() for t in (value, grad, argmax) if t is not None])


def patch_prior_bits(jolideco_amd, brief=False):
    import gmm_jitter_cases
    import gmm_subpix_cases
    from image_norm_cases import fixture_gmm, make_norm
    from jolideco_amd import _hip
    from jolideco_amd.ops import DeviceShifts
    from jolideco_amd.priors.patches import GaussianMixtureModel, GaussianMixtureModelMeta
    from jolideco_amd.utils.norms import StandardizedSubtractMeanPatchNorm
    from tools import gmm16_cases

    cache = {}

    def golden(name):
        if name not in cache:
            cache[name] = dict(np.load(REPO / "tests" / "golden" / f"{name}.npz"))
        return cache[name]

    def model(arrays, stride=4):
        return GaussianMixtureModel.from_numpy(*arrays, meta=GaussianMixtureModelMeta(stride=stride))

    def dev(array, dtype=torch.float32):
        return torch.from_numpy(np.ascontiguousarray(array)).to(device=DEV, dtype=dtype)

    def device_roll(roll, shape):
        roll = (0, 0) if roll is None else roll
        return DeviceShifts(dev([roll[0] % shape[0], roll[1] % shape[1]], torch.int32), roll)

    models = {64: model(gmm_subpix_cases.fixture_gmm(golden)), 256: model(gmm_subpix_cases.mixture256(), gmm16_cases.STRIDE)}
    items = []  # (label, D, flux, stride, {form: (shifts, keywords of the staged pass)})
    for d, rows in ((64, gmm_subpix_cases.CASES), (256, gmm_subpix_cases.CASES_256)):
        for index, (shape, stride, roll, offsets) in enumerate(rows):
            flux = dev(gmm_subpix_cases.case_flux(index, None if d == 64 else rows))
            forms = {"plain": (roll, {}), "subpix": (roll, dict(subpix=offsets)),
                     "subpix-device": (device_roll(roll, shape), dict(subpix=DeviceShifts(dev(offsets), offsets)))}
            items.append((f"subpix/D{d}/case{index}", d, flux, stride, forms))
    for d, rows in ((64, gmm_jitter_cases.CASES), (256, gmm_jitter_cases.CASES_256)):
        for index, (shape, stride, roll) in enumerate(rows):
            flux = dev(gmm_jitter_cases.case_flux(index, d))
            draws = gmm_jitter_cases.case_draws(index, d)
            forms = {"plain": (roll, {}), "jitter-host": (roll, dict(jitter=tuple(torch.from_numpy(j) for j in draws))),
                     "jitter-device": (device_roll(roll, shape), dict(jitter=tuple(dev(j, torch.int32) for j in draws)))}
            items.append((f"jitter/D{d}/case{index}", d, flux, stride, forms))
    norms = {"identity": None, "asinh": make_norm("asinh")}
    patch_norms = {"subtract-mean": None, "std-subtract-mean": StandardizedSubtractMeanPatchNorm()}
    for label, d, flux, stride, forms in items:
        handle = models[d].handle(DEV)
        for mode, screens in (("max", (None,)), ("lse", ("0", "2"))):
            for screen in screens:
                _hip.set_option("JD_GMM_LSE_SCREEN", screen)
                route, lines = f"{label}/{mode}{'' if screen is None else '-screen' + screen}", []
                for (norm_name, norm), (pn_name, patch_norm) in ((n, p) for n in norms.items() for p in patch_norms.items()):
                    for form, (shifts, keywords) in forms.items():
                        for setup in ("grad", "forward", "value"):
                            line = _prior_call_digest(handle, flux, stride, shifts, setup, mode == "lse", norm=norm,
                                                      patch_norm=patch_norm, **keywords)
                            lines.append(f"{route}/{norm_name}/{pn_name}/{form}/{setup}: {line}\n")
                if brief:  # one line per case and route: the sha256 of its per-call lines
                    print(f"{route}: {hashlib.sha256(''.join(lines).encode()).hexdigest()} calls={len(lines)}", flush=True)
                else:
                    print("".join(lines), end="", flush=True)
    _hip.set_option("JD_GMM_LSE_SCREEN", None)

    from conftest import unpack_datasets

    for name, prior_class in (("gmm_subpix", jolideco_amd.SubpixelGMMPatchPrior), ("gmm_jitter", jolideco_amd.JitteredGMMPatchPrior)):
        g = golden(name)
        prior = prior_class(gmm=model(fixture_gmm(golden, "fit/gmm/")))
        comp = jolideco_amd.SpatialFluxComponent.from_numpy(flux=g["fit/flux_init"], prior=prior)
        n_epochs = {"gmm_subpix": gmm_subpix_cases, "gmm_jitter": gmm_jitter_cases}[name].FIT_EPOCHS
        res = jolideco_amd.MAPDeconvolver(n_epochs=n_epochs, display_progress=False, device=DEV).run(
            unpack_datasets(g, "fit/data/"), components=comp)
        print(f"{name}-fit: {digest([np.asarray(res.flux_total), np.asarray(res.trace_loss['total'])])}", flush=True)


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

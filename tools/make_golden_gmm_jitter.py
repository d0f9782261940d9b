"""Generate tests/golden/gmm_jitter.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_gmm_jitter.py

The GMM patch prior with a jittered patch grid.  From the reference's `GMMPatchPrior(cycle_spin=True, jitter=True,
generator=seeded)` on the distinct (shape, stride) of tests/gmm_jitter_cases.CASES and CASES_256, `marginalize` False and
True, plus one case under `ASinhImageNorm` and one with `cycle_spin=False`: the draws (recovered by replaying the generator:
two roll draws, rows first, then the columns' jitter, then the rows'), the value and the autograd gradient.  While generating,
the float32 oracle of tests/gmm_jitter_cases.py is asserted to reproduce the reference within 1e-6 relative on the value and on
the gradient's L-infinity norm -- it is what the GPU tests compare against.  And one 6-epoch sequential fit of a 32 x 32 scene,
two observations, default generators, asserted against `cpu_ref.map_fit_sequential` with the oracle prior class.  The mixtures
are those of tests/golden/image_norm.npz and of tools/gmm16_cases.py; the fixture holds data only.
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
from jolideco.models import SpatialFluxComponent  # noqa: E402
from jolideco.priors import GMMPatchPrior  # noqa: E402
from jolideco.utils import norms as ref_norms  # noqa: E402

import gmm_jitter_cases as cases  # noqa: E402
from jolideco_amd.utils import norms as host_norms  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from tools import gmm16_cases  # noqa: E402

ASINH = {"alpha": 3.0, "beta": 40.0}


def fixture_items():
    """[(tag, table, index, marginalize, asinh norm, cycle_spin)]: every distinct (shape, stride) in both modes, then the two
    extra cases on the first shape"""
    seen, items = set(), []
    for table in (64, 256):
        for index, (shape, stride, _) in enumerate(cases.table_of(table)[0]):
            if (table, shape, stride) in seen:
                continue
            seen.add((table, shape, stride))
            for marginalize in (False, True):
                items.append((f"d{table}/case{index}/{'lse' if marginalize else 'max'}", table, index, marginalize, False, True))
    items.append(("d64/case0/asinh", 64, 0, False, True, True))
    items.append(("d64/case0/no_roll", 64, 0, False, False, False))
    return items


def main():
    torch.manual_seed(0)
    g = dict(np.load(REPO / "tests" / "golden" / "image_norm.npz"))
    arrays64 = tuple(np.asarray(g[f"gmm/{n}"], dtype=np.float64) for n in ("means", "covariances", "weights"))
    out = {}
    for i, (tag, table, index, marginalize, normed, cycle_spin) in enumerate(fixture_items()):
        rows, patch, _ = cases.table_of(table)
        shape, stride, _ = rows[index]
        arrays, meta_stride = (arrays64, cases.GMM_META_STRIDE) if table == 64 else (cases.mixture256(), gmm16_cases.STRIDE)
        flux = cases.case_flux(index, table)
        norm_r = norm_h = None
        kwargs = {}
        if normed:
            norm_r = ref_norms.NORMS_REGISTRY["asinh"](frozen=True, **ASINH)
            for p in torch.nn.Module.parameters(norm_r):
                p.requires_grad_(False)
            norm_h = host_norms.ASinhImageNorm(**ASINH)
            kwargs["norm"] = norm_r
        seed = cases.FIXTURE_SEED + i
        prior = GMMPatchPrior(gmm=mg.ref_gmm(*arrays, stride=meta_stride), stride=stride, cycle_spin=cycle_spin, jitter=True,
                              generator=torch.Generator("cpu").manual_seed(seed), marginalize=marginalize, **kwargs)
        f = torch.from_numpy(flux[None, None]).clone().requires_grad_(True)
        value = prior(f)
        value.backward()
        roll, jitter = cases.draw(torch.Generator("cpu").manual_seed(seed), shape, patch, stride, cycle_spin)
        assert all(np.abs(j).max() <= patch - stride for j in jitter)
        total, grad, _, _ = cases.oracle(flux, norm_h, arrays, patch, stride, roll, jitter, marginalize, np.float32,
                                         meta_stride=meta_stride)
        scale = stride**2 / float(patch * patch) / flux.size
        e_value = abs(total * scale - float(value.detach())) / abs(float(value.detach()))
        e_grad = cases.rel_err(grad * scale, f.grad.numpy()[0, 0])
        assert e_value <= 1e-6 and e_grad <= 1e-6, (tag, e_value, e_grad)
        out[f"{tag}/table"] = np.int64(table)
        out[f"{tag}/index"] = np.int64(index)
        out[f"{tag}/seed"] = np.int64(seed)
        out[f"{tag}/roll"] = np.array([-99, -99] if roll is None else roll, dtype=np.int64)
        out[f"{tag}/jitter_y"] = jitter[0]
        out[f"{tag}/jitter_x"] = jitter[1]
        out[f"{tag}/value"] = np.float64(value.detach())
        out[f"{tag}/grad"] = f.grad.numpy()[0, 0]
        print("gmm_jitter", tag, shape, "roll", roll, "jitter", jitter, f"oracle vs reference: value {e_value:.1e} gradient {e_grad:.1e}")
    out["tags"] = np.array([item[0] for item in fixture_items()])

    # the fit: 32 x 32 scene, two observations, default generators, the K = 6 mixture of the image-norm fit
    farrays = tuple(np.asarray(g[f"fit/gmm/{n}"], dtype=np.float64) for n in ("means", "covariances", "weights"))
    rs = np.random.RandomState(cases.FIT_SEED)
    datasets = {f"o{i}": mg.scene(cases.FIT_SHAPE, mg.asym_psf((7, 7), 1.2 + 0.3 * i, 1.6), rs, n_points=4, bkg=0.8)
                for i in range(2)}
    flux_init = rs.gamma(30, size=cases.FIT_SHAPE)
    comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=GMMPatchPrior(gmm=mg.ref_gmm(*farrays), jitter=True))
    res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False).run(datasets=datasets, components=comp)
    oracle_prior = cases.JitterPatchPriorRef(cpu_ref.GMM.from_numpy(*farrays, stride=4))
    final, trace = cpu_ref.map_fit_sequential(datasets, {"flux": flux_init}, {"flux": oracle_prior}, n_epochs=cases.FIT_EPOCHS)
    e_flux = cases.rel_err(final["flux"], res.flux_total)
    assert e_flux <= 1e-6, e_flux
    assert abs(trace[-1]["total"] - res.trace_loss[-1]["total"]) <= 1e-6 * abs(res.trace_loss[-1]["total"])
    out.update({f"fit/{k}": v for k, v in mg.pack_datasets(datasets).items()})
    out.update({"fit/flux_init": flux_init, "fit/flux_final": res.flux_total})
    out.update({f"fit/{k}": v for k, v in mg.trace_to_arrays(res.trace_loss).items()})
    print("gmm_jitter fit ok", res.trace_loss[-1]["total"], f"oracle vs reference: flux {e_flux:.1e}")

    path = REPO / "tests" / "golden" / "gmm_jitter.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

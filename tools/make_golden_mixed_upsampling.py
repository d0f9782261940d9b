"""Generate tests/golden/mixed_upsampling.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_mixed_upsampling.py

Two flux components with DIFFERENT up-sampling factors in one fit (`upsampling_factor` is an attribute of each
SpatialFluxComponent; NPredModels.from_dataset_numpy builds one NPredModel per component with that component's factor,
jolideco/models/npred.py:279-295).  The helpers -- reference loader, scene, PSFs, GMM, packing -- are those of
oracle/refload/make_golden.py, imported as a module.  The fixture holds data only: inputs, final up-sampled fluxes per
component, trace columns, and one step's npred / d loss / d flux_c.  While generating, oracle/cpu_ref.py is asserted to
reproduce the reference bit for bit.
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

from jolideco.core import MAPDeconvolver  # noqa: E402
from jolideco.models import FluxComponents, NPredModels, SpatialFluxComponent  # noqa: E402
from jolideco.priors import GMMPatchPrior, InverseGammaPrior  # noqa: E402

from oracle import cpu_ref  # noqa: E402

SHAPE = (40, 44)
N_EPOCHS = 4
PAIRS = ((1, 2), (3, 2))  # (factor of "extended", factor of "points")


def inputs():
    rs = np.random.RandomState(57)
    means, covs, weights = cpu_ref.synthetic_gmm(6, 64, seed=12)
    datasets = {}
    for i in range(2):
        d = mg.scene(SHAPE, mg.asym_psf((9, 9), 2.5 + 0.5 * i, 3.0), rs, bkg=0.6)
        small = np.ones((5, 5)) + 0.3 * rs.uniform(size=(5, 5))
        d["psf"] = {"extended": d["psf"], "points": (small / small.sum()).astype(np.float32)}
        datasets[f"o{i}"] = d
    init_ext = rs.gamma(30, size=SHAPE)
    init_pts = rs.gamma(2, size=SHAPE) * 0.2
    return datasets, (means, covs, weights), init_ext, init_pts


def components(gmm, init_ext, init_pts, u_ext, u_pts):
    comps = FluxComponents()
    comps["extended"] = SpatialFluxComponent.from_numpy(
        flux=init_ext, upsampling_factor=u_ext, prior=GMMPatchPrior(gmm=mg.ref_gmm(*gmm))
    )
    comps["points"] = SpatialFluxComponent.from_numpy(
        flux=init_pts, upsampling_factor=u_pts, prior=InverseGammaPrior(alpha=10, beta=1.5)
    )
    return comps


def main():
    torch.manual_seed(0)
    datasets, gmm, init_ext, init_pts = inputs()
    out = {"gmm/means": gmm[0], "gmm/covariances": gmm[1], "gmm/weights": gmm[2], "init/extended": init_ext,
           "init/points": init_pts}
    out.update(mg.pack_datasets(datasets))
    gmm_o = cpu_ref.GMM.from_numpy(*gmm, stride=4)
    for u_ext, u_pts in PAIRS:
        tag = f"u{u_ext}{u_pts}"
        comps = components(gmm, init_ext, init_pts, u_ext, u_pts)
        res = MAPDeconvolver(n_epochs=N_EPOCHS, display_progress=False).run(datasets=datasets, components=comps)
        final, trace = cpu_ref.map_fit_sequential(
            datasets, {"extended": init_ext, "points": init_pts},
            {"extended": cpu_ref.GMMPatchPriorRef(gmm_o), "points": cpu_ref.InverseGammaPriorRef(10, 1.5)},
            n_epochs=N_EPOCHS, upsampling_factors={"extended": u_ext, "points": u_pts},
        )
        up = {name: comp.flux_upsampled.detach().numpy()[0, 0] for name, comp in res.components.items()}
        assert up["extended"].shape == (SHAPE[0] * u_ext, SHAPE[1] * u_ext)
        assert up["points"].shape == (SHAPE[0] * u_pts, SHAPE[1] * u_pts)
        assert res.flux_total.shape == SHAPE
        assert np.array_equal(final["extended"], up["extended"]) and np.array_equal(final["points"], up["points"])
        assert trace[-1]["total"] == res.trace_loss[-1]["total"]
        out[f"{tag}/final_upsampled/extended"] = up["extended"]
        out[f"{tag}/final_upsampled/points"] = up["points"]
        out[f"{tag}/flux_total"] = res.flux_total
        out.update({f"{tag}/{k}": v for k, v in mg.trace_to_arrays(res.trace_loss).items()})
        print("mixed_upsampling", tag, "ok", res.trace_loss[-1]["total"])

    # one step's npred and d loss / d flux_c for (1, 2): NPredModels.evaluate + PoissonNLLLoss autograd on dataset o0
    comps = components(gmm, init_ext, init_pts, 1, 2)
    models = NPredModels.from_dataset_numpy(dataset=datasets["o0"], components=comps)
    fluxes = tuple(f.detach().clone().requires_grad_(True) for f in comps.to_flux_tuple())
    npred = models.evaluate(fluxes=fluxes)
    loss_fn = torch.nn.PoissonNLLLoss(log_input=False, reduction="mean", eps=1e-25, full=True)
    loss = loss_fn(npred, torch.from_numpy(datasets["o0"]["counts"][None, None]))
    loss.backward()
    d = cpu_ref.DatasetRef.from_numpy(datasets["o0"], ["extended", "points"], [1, 2])
    fluxes_o = tuple(f.detach().clone().requires_grad_(True) for f in fluxes)
    loss_o = d.loss(fluxes_o)
    loss_o.backward()
    assert float(loss_o.detach()) == float(loss.detach()) and np.array_equal(d.npred(fluxes_o).detach().numpy(), npred.detach().numpy())
    for f, fo in zip(fluxes, fluxes_o):
        assert np.array_equal(f.grad.numpy(), fo.grad.numpy())
    out["step/flux/extended"] = fluxes[0].detach().numpy()[0, 0]
    out["step/flux/points"] = fluxes[1].detach().numpy()[0, 0]
    out["step/npred"] = npred.detach().numpy()[0, 0]
    out["step/loss"] = np.float64(loss.detach())
    out["step/grad_flux/extended"] = fluxes[0].grad.numpy()[0, 0]
    out["step/grad_flux/points"] = fluxes[1].grad.numpy()[0, 0]

    path = REPO / "tests" / "golden" / "mixed_upsampling.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

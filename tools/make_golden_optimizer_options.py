"""Generate tests/golden/optimizer_options.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_optimizer_options.py

Two 6-epoch fits of a 32 x 32 scene with two observations and trainable calibrations, with options of torch.optim in
`optimizer_kwargs` -- the reference hands them to torch.optim.Adam / torch.optim.SGD unchanged (jolideco/core.py:202-204),
ONE optimizer over the flux and every calibration parameter:
  adam/  sequential (`MAPDeconvolver.run`), GMM patch prior (6 synthetic components), Adam {weight_decay: 1e-2, amsgrad: True}
  sgd/   joint (one step per epoch on sum_d L_d - beta * logprior, the harness of oracle/refload/make_golden.py
         `joint_and_multi` from the reference's own pieces), InverseGammaPrior, SGD {momentum: 0.9, nesterov: True} at
         learning rate 1e-3
The fixture holds data only: inputs, final fluxes, final calibrations, trace columns.
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
from jolideco.loss import TotalLoss  # noqa: E402
from jolideco.models import FluxComponents, NPredCalibration, NPredCalibrations, SpatialFluxComponent  # noqa: E402
from jolideco.priors import GMMPatchPrior, InverseGammaPrior  # noqa: E402

from oracle import cpu_ref  # noqa: E402

SHAPE = (32, 32)
N_EPOCHS = 6
ADAM_KWARGS = {"weight_decay": 1e-2, "amsgrad": True}
SGD_KWARGS = {"momentum": 0.9, "nesterov": True}
SGD_LR = 1e-3
CALIBRATIONS = {
    "o0": dict(shift_x=0.3, shift_y=-0.2, background_norm=1.2, psf_scale=1.0),
    "o1": dict(shift_x=-0.15, shift_y=0.25, background_norm=0.9, psf_scale=1.0),
}


def inputs(seed):
    rs = np.random.RandomState(seed)
    datasets = {f"o{i}": mg.scene(SHAPE, mg.asym_psf((7, 7), 1.2 + 0.3 * i, 1.6), rs, n_points=4, bkg=0.8 + 0.1 * i) for i in range(2)}
    cals = NPredCalibrations()
    for name, kw in CALIBRATIONS.items():
        cals[name] = NPredCalibration(**kw)
    return datasets, rs.gamma(30, size=SHAPE), cals


def pack(tag, datasets, flux_init, flux_final, cals, trace_arrays):
    out = {f"{tag}/flux_init": flux_init, f"{tag}/flux_final": flux_final}
    out.update({f"{tag}/{k}": v for k, v in mg.pack_datasets(datasets).items()})
    out.update({f"{tag}/{k}": v for k, v in trace_arrays.items()})
    for name, kw in CALIBRATIONS.items():
        out[f"{tag}/cal_init/{name}"] = np.array([kw["shift_x"], kw["shift_y"], kw["background_norm"], kw["psf_scale"]])
        d = cals[name].to_dict()
        out[f"{tag}/cal_final/{name}"] = np.array([d["shift_x"], d["shift_y"], d["background_norm"], d["psf_scale"]])
        assert d["shift_x"] != kw["shift_x"] and d["background_norm"] != kw["background_norm"], name  # (they were trained)
    return out


def adam_fit():
    datasets, flux_init, cals = inputs(611)
    means, covs, weights = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in cpu_ref.synthetic_gmm(6, 64, seed=23))
    comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=GMMPatchPrior(gmm=mg.ref_gmm(means, covs, weights)))
    deconvolver = MAPDeconvolver(n_epochs=N_EPOCHS, display_progress=False, optimizer_kwargs=dict(ADAM_KWARGS))
    res = deconvolver.run(datasets=datasets, components=comp, calibrations=cals)
    group = deconvolver.optimizer.param_groups[0]
    assert isinstance(deconvolver.optimizer, torch.optim.Adam) and group["amsgrad"] is True and group["weight_decay"] == 1e-2
    assert all("max_exp_avg_sq" in state for state in deconvolver.optimizer.state.values())
    out = pack("adam", datasets, flux_init, res.flux_upsampled_total, res.calibrations, mg.trace_to_arrays(res.trace_loss))
    out.update({"adam/gmm/means": means.astype(np.float32), "adam/gmm/covariances": covs.astype(np.float32),
                "adam/gmm/weights": weights.astype(np.float32)})
    print("optimizer_options adam ok", res.trace_loss[-1]["total"], res.calibrations["o0"].to_dict())
    return out


def sgd_fit():
    datasets, flux_init, cals = inputs(612)
    comps = FluxComponents()
    comps["flux"] = SpatialFluxComponent.from_numpy(flux=flux_init, prior=InverseGammaPrior(alpha=10, beta=1.5))
    total_loss = TotalLoss.from_datasets_and_components(datasets=datasets, components=comps, calibrations=cals, beta=1.0)
    parameters = list(comps.parameters()) + list(cals.parameters())  # (jolideco/core.py:197-204)
    opt = torch.optim.SGD(parameters, lr=SGD_LR, **SGD_KWARGS)
    rows = []
    for _ in range(N_EPOCHS):
        opt.zero_grad()
        fluxes = comps.to_flux_tuple()
        losses = [total_loss.poisson_loss.loss_function(m.evaluate(fluxes=fluxes), c) for c, m in total_loss.poisson_loss.iter_by_dataset]
        lp = total_loss.prior_loss.evaluate(fluxes=fluxes)
        (sum(losses) - 1.0 * sum(lp)).backward()
        opt.step()
        rows.append(cpu_ref._trace_row(list(datasets), ["flux"], [v.item() for v in losses], [v.item() for v in lp], 1.0))
    stepped = [p for p in parameters if "momentum_buffer" in opt.state.get(p, {})]
    assert len(stepped) == 1 + 2 * len(CALIBRATIONS), len(stepped)  # (the flux and every shift / background norm)
    flux_final = comps["flux"].flux_upsampled.detach().numpy()[0, 0]
    out = pack("sgd", datasets, flux_init, flux_final, cals, mg.rows_to_arrays(rows))
    print("optimizer_options sgd ok", rows[-1]["total"], cals["o0"].to_dict())
    return out


def main():
    torch.manual_seed(0)
    out = {"n_epochs": np.int64(N_EPOCHS), "sgd/lr": np.float64(SGD_LR)}
    out.update(adam_fit())
    out.update(sgd_fit())
    path = REPO / "tests" / "golden" / "optimizer_options.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

"""Generate tests/golden/image_norm.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_image_norm.py

The image norms of the GMM patch prior (jolideco/utils/norms.py:225-426, applied at priors/patches/core.py:190).  For
each of the six norms this package implements, with non-default parameters: the normed image, the prior value for
`marginalize` False / True and the autograd gradient with respect to the flux, all from the reference's
`GMMPatchPrior(norm=..., cycle_spin=False)`; plus a 10-epoch sequential fit under `ASinhImageNorm()`.  The reference's
norm parameters are constants everywhere (`requires_grad_(False)`, `frozen=True`): this package does not train them.
While generating, `oracle/cpu_ref.gmm_patch_log_prior(norm(flux), ...)` with the host norm classes of
jolideco_amd.utils.norms is asserted to reproduce the reference -- that composition is the oracle of the GPU tests.
The fixture holds data only.
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
from jolideco.models import SpatialFluxComponent  # noqa: E402
from jolideco.priors import GMMPatchPrior  # noqa: E402
from jolideco.utils import norms as ref_norms  # noqa: E402

from jolideco_amd.utils import norms as host_norms  # noqa: E402
from oracle import cpu_ref  # noqa: E402

SHAPE = (40, 44)
STRIDE = 4
K = 12
# type -> constructor arguments (non-default; the flux is gamma(20): values of roughly 8 .. 40)
NORM_CASES = {
    "asinh": {"alpha": 3.0, "beta": 40.0},
    "fixed-max": {"max_value": 24.0},  # clips about a fifth of the pixels
    "sigmoid": {"alpha": 6.0, "beta": 40.0},
    "atan": {"alpha": 15.0},
    "log": {"alpha": 2.5},
    "power": {"alpha": 0.6, "beta": 30.0},
}
FIT_SHAPE = (32, 32)
FIT_EPOCHS = 10


def frozen_ref_norm(type_, kwargs):
    norm = ref_norms.NORMS_REGISTRY[type_](frozen=True, **kwargs)
    for p in torch.nn.Module.parameters(norm):  # (norm.parameters() of a frozen norm is empty)
        p.requires_grad_(False)
    return norm


def float32_exact(means, covs, weights):
    """The mixture rounded to float32 BEFORE anyone sees it (stored as float32: half the fixture's size)"""
    return tuple(np.asarray(a, dtype=np.float32).astype(np.float64) for a in (means, covs, weights))


class NormedPriorRef:
    """oracle prior on norm(flux): the composition the GPU tests compare against"""

    def __init__(self, prior, norm):
        self.prior, self.norm = prior, norm

    def __call__(self, flux):
        return self.prior(self.norm(flux))


def main():
    torch.manual_seed(0)
    rs = np.random.RandomState(2310)
    flux = rs.gamma(20, size=SHAPE).astype(np.float32)
    means, covs, weights = float32_exact(*cpu_ref.synthetic_gmm(K, 64, seed=31))
    gmm_o = cpu_ref.GMM.from_numpy(means, covs, weights, stride=STRIDE)
    out = {"flux": flux, "gmm/means": means.astype(np.float32), "gmm/covariances": covs.astype(np.float32),
           "gmm/weights": weights.astype(np.float32),
           "stride": np.int64(STRIDE), "types": np.array(list(NORM_CASES))}
    for type_, kwargs in NORM_CASES.items():
        norm_r = frozen_ref_norm(type_, kwargs)
        norm_h = host_norms.NORMS_REGISTRY[type_](**kwargs)
        assert norm_r.to_dict() == norm_h.to_dict(), (norm_r.to_dict(), norm_h.to_dict())
        out[f"{type_}/params"] = np.array([kwargs.get("max_value", kwargs.get("alpha", 0.0)), kwargs.get("beta", 0.0)])
        image = torch.from_numpy(flux[None, None])
        normed = norm_r(image).detach().numpy()[0, 0]
        assert np.array_equal(normed, norm_h(image).numpy()[0, 0]), type_
        out[f"{type_}/normed"] = normed
        for marginalize in (False, True):
            prior = GMMPatchPrior(gmm=mg.ref_gmm(means, covs, weights, stride=STRIDE), norm=norm_r, cycle_spin=False,
                                  marginalize=marginalize, stride=STRIDE)
            f = image.clone().requires_grad_(True)
            value = prior(f)
            value.backward()
            fo = image.clone().requires_grad_(True)
            value_o = cpu_ref.gmm_patch_log_prior(norm_h(fo), gmm_o, STRIDE, None, marginalize=marginalize)
            value_o.backward()
            # cpu_ref.gmm_patch_log_prior divides by numel of what it is given (the normed image: the same number)
            assert float(value_o.detach()) == float(value.detach()), (type_, marginalize)
            assert np.array_equal(fo.grad.numpy(), f.grad.numpy()), (type_, marginalize)
            tag = f"{type_}/{'lse' if marginalize else 'max'}"
            out[f"{tag}/value"] = np.float64(value.detach())
            out[f"{tag}/grad"] = f.grad.numpy()[0, 0]
        print("image_norm", type_, "ok", float(out[f"{type_}/max/value"]), float(out[f"{type_}/lse/value"]))

    # the fit: 32 x 32 scene, upsampling_factor 2, asinh norm with its default parameters
    rs = np.random.RandomState(99)
    datasets = {f"o{i}": mg.scene(FIT_SHAPE, mg.asym_psf((7, 7), 1.5 + 0.5 * i, 2.0), rs, bkg=0.8) for i in range(2)}
    flux_init = rs.gamma(30, size=FIT_SHAPE)
    fmeans, fcovs, fweights = float32_exact(*cpu_ref.synthetic_gmm(6, 64, seed=17))
    norm_r = frozen_ref_norm("asinh", {})
    comp = SpatialFluxComponent.from_numpy(
        flux=flux_init, upsampling_factor=2, prior=GMMPatchPrior(gmm=mg.ref_gmm(fmeans, fcovs, fweights), norm=norm_r)
    )
    res = MAPDeconvolver(n_epochs=FIT_EPOCHS, display_progress=False).run(datasets=datasets, components=comp)
    assert float(norm_r.alpha) == 1.0 and float(norm_r.beta) == 1.0  # (constants: nothing trained them)
    gmm_f = cpu_ref.GMM.from_numpy(fmeans, fcovs, fweights, stride=4)
    final, trace = cpu_ref.map_fit_sequential(
        datasets, {"flux": flux_init}, {"flux": NormedPriorRef(cpu_ref.GMMPatchPriorRef(gmm_f), host_norms.ASinhImageNorm())},
        n_epochs=FIT_EPOCHS, upsampling_factors={"flux": 2},
    )
    up = res.components["flux"].flux_upsampled.detach().numpy()[0, 0]
    assert np.array_equal(final["flux"], up), np.abs(final["flux"] - up).max()
    assert trace[-1]["total"] == res.trace_loss[-1]["total"]
    out.update({f"fit/{k}": v for k, v in mg.pack_datasets(datasets).items()})
    out.update({"fit/flux_init": flux_init, "fit/flux_upsampled_final": up, "fit/flux_final": res.flux_total,
                "fit/gmm/means": fmeans.astype(np.float32), "fit/gmm/covariances": fcovs.astype(np.float32),
                "fit/gmm/weights": fweights.astype(np.float32)})
    out.update({f"fit/{k}": v for k, v in mg.trace_to_arrays(res.trace_loss).items()})
    print("image_norm fit ok", res.trace_loss[-1]["total"])

    path = REPO / "tests" / "golden" / "image_norm.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

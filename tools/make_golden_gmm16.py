"""Generate tests/golden/gmm16.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_gmm16.py

The GMM patch prior on 16x16 patches (256 features; jolideco/priors/patches/core.py:180-246 is written for any square
patch, and the reference ships a 16x16 mixture with stride 8).  From the reference's `GMMPatchPrior(cycle_spin=False)` on a
48 x 56 gamma-distributed flux with one pixel at -2e5 (the one patch that covers it is filtered by `> -1e5`): value and
autograd gradient for `marginalize` False / True, bare and under a frozen `ASinhImageNorm`; the (N, K) matrix of
`estimate_log_prob` on the mean-free patches of the clean flux; and a 6-epoch sequential fit of a 48 x 48 scene with
cycle-spin on and the default generator.  While generating, `oracle/cpu_ref` (`gmm_patch_log_prior`, `gmm_log_prob`,
`map_fit_sequential`) is asserted to reproduce the reference exactly on every case -- that composition is the oracle of
the GPU tests.

The mixtures are `cpu_ref.synthetic_gmm(K, 256, seed, zero_means=False)` rounded to float32.  Their covariances alone
would be 1.3 MB, so the fixture stores the seed, K and a float64 checksum; the tests rebuild them and assert the checksum.
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

from tools import gmm16_cases as cases  # noqa: E402  (the constants and the mixture builder the tests use)


def frozen_ref_norm(type_, kwargs):
    norm = ref_norms.NORMS_REGISTRY[type_](frozen=True, **kwargs)
    for p in torch.nn.Module.parameters(norm):  # (norm.parameters() of a frozen norm is empty)
        p.requires_grad_(False)
    return norm


def main():
    torch.manual_seed(0)
    flux_clean = cases.fixture_flux(filtered=False)
    flux = cases.fixture_flux(filtered=True)
    arrays = cases.synthetic_mixture(cases.K, cases.SEED)
    out = {"flux": flux, "K": np.int64(cases.K), "seed": np.int64(cases.SEED), "stride": np.int64(cases.STRIDE),
           "gmm/checksum": np.float64(cases.mixture_checksum(arrays)),
           "asinh/params": np.array([cases.ASINH["alpha"], cases.ASINH["beta"]])}
    gmm_o = cpu_ref.GMM.from_numpy(*arrays, stride=cases.STRIDE)
    image = torch.from_numpy(flux[None, None])
    for tag_norm in ("bare", "asinh"):
        norm_r = frozen_ref_norm("asinh", cases.ASINH) if tag_norm == "asinh" else None
        norm_h = host_norms.ASinhImageNorm(**cases.ASINH) if tag_norm == "asinh" else (lambda t: t)
        for marginalize in (False, True):
            kwargs = {} if norm_r is None else {"norm": norm_r}
            prior = GMMPatchPrior(gmm=mg.ref_gmm(*arrays, stride=cases.STRIDE), cycle_spin=False, marginalize=marginalize,
                                  stride=cases.STRIDE, **kwargs)
            assert tuple(prior.patch_shape) == (16, 16)
            f = image.clone().requires_grad_(True)
            value = prior(f)
            value.backward()
            fo = image.clone().requires_grad_(True)
            value_o = cpu_ref.gmm_patch_log_prior(norm_h(fo), gmm_o, cases.STRIDE, None, marginalize=marginalize)
            value_o.backward()
            assert float(value_o.detach()) == float(value.detach()), (tag_norm, marginalize)
            assert np.array_equal(fo.grad.numpy(), f.grad.numpy()), (tag_norm, marginalize)
            tag = f"{tag_norm}/{'lse' if marginalize else 'max'}"
            out[f"{tag}/value"] = np.float64(value.detach())
            out[f"{tag}/grad"] = f.grad.numpy()[0, 0]
            print("gmm16", tag, "ok", float(value.detach()))

    # (N, K) log-probabilities of explicit patches
    x = cases.mean_free_patches(flux_clean, cases.STRIDE)
    ref = mg.ref_gmm(*arrays, stride=cases.STRIDE)
    logp = ref.estimate_log_prob(torch.from_numpy(x)).detach().numpy()
    logp_o = cpu_ref.gmm_log_prob(torch.from_numpy(x), gmm_o).numpy()
    assert np.array_equal(logp, logp_o)
    out["log_prob"] = logp
    print("gmm16 log_prob ok", logp.shape)

    # the fit: 48 x 48 scene, cycle-spin on, default generator
    rs = np.random.RandomState(cases.FIT_SEED)
    datasets = {f"o{i}": mg.scene(cases.FIT_SHAPE, mg.asym_psf((7, 7), 1.5 + 0.5 * i, 2.0), rs, bkg=0.8) for i in range(2)}
    flux_init = rs.gamma(30, size=cases.FIT_SHAPE)
    farrays = cases.synthetic_mixture(cases.FIT_K, cases.FIT_GMM_SEED)
    comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=GMMPatchPrior(gmm=mg.ref_gmm(*farrays, stride=cases.STRIDE)))
    res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False).run(datasets=datasets, components=comp)
    gmm_f = cpu_ref.GMM.from_numpy(*farrays, stride=cases.STRIDE)
    final, trace = cpu_ref.map_fit_sequential(
        datasets, {"flux": flux_init}, {"flux": cpu_ref.GMMPatchPriorRef(gmm_f)}, n_epochs=cases.FIT_EPOCHS
    )
    assert np.array_equal(final["flux"], res.flux_total), np.abs(final["flux"] - res.flux_total).max()
    assert trace[-1]["total"] == res.trace_loss[-1]["total"]
    out.update({f"fit/{k}": v for k, v in mg.pack_datasets(datasets).items()})
    out.update({"fit/flux_init": flux_init, "fit/flux_final": res.flux_total, "fit/K": np.int64(cases.FIT_K),
                "fit/seed": np.int64(cases.FIT_GMM_SEED), "fit/gmm/checksum": np.float64(cases.mixture_checksum(farrays))})
    out.update({f"fit/{k}": v for k, v in mg.trace_to_arrays(res.trace_loss).items()})
    print("gmm16 fit ok", res.trace_loss[-1]["total"])

    path = REPO / "tests" / "golden" / "gmm16.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

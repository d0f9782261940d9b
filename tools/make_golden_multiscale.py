"""Generate tests/golden/multiscale.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_multiscale.py

`jolideco.priors.MultiScalePrior` (jolideco/priors/patches/core.py:249-337) works with ``cycle_spin=False`` only: with the
default ``cycle_spin=True`` its ``flux, _ = cycle_spin(...)`` unpacks a tensor and raises ValueError (asserted here).  For
every case of tests/multiscale_cases.py the reference can run -- its ``_log_weights`` frozen, as the image norms'
parameters are elsewhere -- the fixture holds the reference's value and autograd gradient and the draws of its inner
prior; for the outer cycle-spin cases it holds the float32 restatement's numbers, marked as such.

While generating, the float32 restatement of tests/multiscale_cases.py is asserted to reproduce the reference's value and
gradient EXACTLY on every case it can run, with the blur taken through the FFT as the reference takes it
(`multiscale_cases.conv_same_fft`).  The tests use the same restatement with the taps summed directly (what the kernels
do); the distance of that form and of the reference from the float64 restatement is printed per case (the tests measure
it again: it is their tolerance).  The kernel array of `multiscale_cases.gaussian_kernel` is asserted equal to the array
the reference convolves with.  The 6-epoch sequential fit is the reference's own `MAPDeconvolver.run`.

The fixture holds data only: mixtures by seed and checksum, small images, draws, margins.
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

from astropy.convolution import Gaussian2DKernel  # noqa: E402
from jolideco.core import MAPDeconvolver  # noqa: E402
from jolideco.models import SpatialFluxComponent  # noqa: E402
from jolideco.priors import GMMPatchPrior, MultiScalePrior  # noqa: E402
from jolideco.utils import norms as ref_norms  # noqa: E402

import multiscale_cases as cases  # noqa: E402
from oracle import cpu_ref  # noqa: E402


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def reference_prior(case, n_levels=None, outer_spin=False, generator=None):
    arrays = cases.case_mixture(case)
    kwargs = {}
    if case["norm"] is not None:
        norm = ref_norms.NORMS_REGISTRY[case["norm"]](frozen=True, **cases.ASINH)
        for p in torch.nn.Module.parameters(norm):
            p.requires_grad_(False)
        kwargs["norm"] = norm
    if generator is None and case["inner_seed"] is not None:
        generator = torch.Generator(device="cpu")
        generator.manual_seed(case["inner_seed"])
    if generator is not None:
        kwargs["generator"] = generator
    inner = GMMPatchPrior(gmm=mg.ref_gmm(*arrays, stride=case["stride"]), cycle_spin=case["inner_spin"],
                          marginalize=case["marginalize"], stride=case["stride"], **kwargs)
    weights = None if case["weights"] is None else torch.tensor(case["weights"])
    prior = MultiScalePrior(prior=inner, n_levels=case["n_levels"] if n_levels is None else n_levels, weights=weights,
                            cycle_spin=outer_spin, anti_alias=case["anti_alias"])
    prior._log_weights.requires_grad_(False)
    return prior


def main():
    torch.manual_seed(0)
    out = {}
    for level in range(cases.MAX_LEVELS):
        sigma = 2 * 2**level / 6.0
        assert np.array_equal(Gaussian2DKernel(sigma).array, cases.gaussian_kernel(sigma)), level
    for name, case in cases.CASES.items():
        flux_np = cases.case_flux(case)
        shifts = cases.draws(case)
        o32, o64 = cases.restate(case, np.float32), cases.restate(case, np.float64)
        out[f"{name}/flux"] = flux_np
        out[f"{name}/gmm_checksum"] = np.float64(cases.mixture_checksum(cases.case_mixture(case)))
        out[f"{name}/draws"] = np.array([(-99, -99) if s is None else s for s in shifts], dtype=np.int64)
        if not case["marginalize"]:
            out[f"{name}/min_margin"] = np.float64(cases.margins(o64["levels"]).min())
        if case["outer_spin"]:
            with np.testing.assert_raises(ValueError):  # the reference's line unpacks one tensor into two names
                reference_prior(case, outer_spin=True)(torch.from_numpy(flux_np[None, None]))
            out[f"{name}/from_reference"] = np.bool_(False)
            out[f"{name}/value"], out[f"{name}/grad"] = np.float64(o32["value"]), o32["grad"].astype(np.float32)
            print("multiscale", name, "restatement only", o32["value"])
            continue
        prior = reference_prior(case)
        f = torch.from_numpy(flux_np[None, None]).clone().requires_grad_(True)
        value = prior(f)
        value.backward()
        grad = f.grad.numpy()[0, 0]
        assert np.array_equal(np.asarray(prior.weights.detach()), np.asarray(cases.level_weights(case["n_levels"], case["weights"])))
        ev, eg = abs(float(value.detach()) - o64["value"]) / abs(o64["value"]), rel_linf(grad, o64["grad"])
        rv, rg = abs(o32["value"] - o64["value"]) / abs(o64["value"]), rel_linf(o32["grad"], o64["grad"])
        print(f"multiscale {name}: value {float(value.detach()):.9g}; against float64: reference {ev:.1e} / {eg:.1e}, "
              f"restatement {rv:.1e} / {rg:.1e} (value / gradient)")
        fft32 = cases.restate(case, np.float32, conv=cases.conv_same_fft)
        assert float(value.detach()) == fft32["value"] and np.array_equal(grad, fft32["grad"].astype(np.float32)), name
        out[f"{name}/from_reference"] = np.bool_(True)
        out[f"{name}/value"], out[f"{name}/grad"] = np.float64(value.detach()), grad

    # the fit: the reference's own run, inner cycle spin with the default generator
    datasets, flux_init, arrays = cases.fit_inputs()
    fit = cases.FIT
    inner = GMMPatchPrior(gmm=mg.ref_gmm(*arrays, stride=fit["stride"]), stride=fit["stride"])
    prior = MultiScalePrior(prior=inner, n_levels=fit["n_levels"], cycle_spin=False)
    prior._log_weights.requires_grad_(False)
    comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=prior)
    res = MAPDeconvolver(n_epochs=fit["n_epochs"], display_progress=False).run(datasets=datasets, components=comp)
    gmm_o = cpu_ref.GMM.from_numpy(*arrays, stride=fit["stride"])
    final, trace = cpu_ref.map_fit_sequential(
        datasets, {"flux": flux_init}, {"flux": cases.MultiScalePriorRef(gmm_o, fit["stride"], fit["n_levels"])},
        n_epochs=fit["n_epochs"],
    )
    final_fft, trace_fft = cpu_ref.map_fit_sequential(
        datasets, {"flux": flux_init},
        {"flux": cases.MultiScalePriorRef(gmm_o, fit["stride"], fit["n_levels"], conv=cases.conv_same_fft)}, n_epochs=fit["n_epochs"],
    )
    assert np.array_equal(final_fft["flux"], res.flux_total), np.abs(final_fft["flux"] - res.flux_total).max()
    assert trace_fft[-1]["total"] == res.trace_loss[-1]["total"]
    err = rel_linf(final["flux"], res.flux_total)
    print(f"multiscale fit: restatement against the reference's run {err:.1e}; total {res.trace_loss[-1]['total']:.9g} / "
          f"{trace[-1]['total']:.9g}")
    assert err < 1e-5 and abs(trace[-1]["total"] - res.trace_loss[-1]["total"]) < 2e-5 * abs(trace[-1]["total"])
    out.update({f"fit/{k}": v for k, v in mg.pack_datasets(datasets).items()})
    out.update({"fit/flux_init": flux_init, "fit/flux_final": res.flux_total,
                "fit/gmm_checksum": np.float64(cases.mixture_checksum(arrays))})
    out.update({f"fit/{k}": v for k, v in mg.trace_to_arrays(res.trace_loss).items()})

    path = REPO / "tests" / "golden" / "multiscale.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

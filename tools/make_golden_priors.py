"""Generate tests/golden/priors.npz from the LIVE reference (build container only).

Run:  python tools/make_golden_priors.py

The priors of a point-source layer.  From the reference's `InverseGammaPrior` / `ExponentialPrior` with
`cycle_spin_subpix=True` and a seeded CPU generator, on a 24 x 40 gamma-distributed flux: the drawn (x0, y0) (recovered by
replaying the generator), the value and the autograd gradient.  From `SmoothnessPrior(width=2)` and `(width=1.5)`: the kernel
array, value and gradient on the same flux.  And two 6-epoch sequential fits of a 32 x 32 scene, one with
`InverseGammaPrior(cycle_spin_subpix=True)` and default generators, one with `SmoothnessPrior()`.  While generating, the
oracles of tests/prior_cases.py are asserted to reproduce the reference on every case -- they are what the GPU tests compare
against.  The fixture holds data only.
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
from jolideco.priors import ExponentialPrior, InverseGammaPrior, SmoothnessPrior  # noqa: E402

import prior_cases as cases  # noqa: E402
from oracle import cpu_ref  # noqa: E402


def main():
    torch.manual_seed(0)
    flux = cases.fixture_flux()
    out = {"flux": flux}
    image = torch.from_numpy(flux[None, None])

    for kind, cls in (("inverse-gamma", InverseGammaPrior), ("exponential", ExponentialPrior)):
        generator = torch.Generator("cpu").manual_seed(cases.FIXTURE_SEED)
        prior = cls(cycle_spin_subpix=True, generator=generator, **cases.SPARSE_PARAMS[kind])
        f = image.clone().requires_grad_(True)
        value = prior(f)
        value.backward()
        x0, y0 = cases.draw_offsets(torch.Generator("cpu").manual_seed(cases.FIXTURE_SEED))
        assert -0.5 <= x0 <= 0.5 and -0.5 <= y0 <= 0.5
        value_o, grad_o = cases.sparse_oracle(flux, kind, x0, y0, dtype=np.float32)
        assert value_o == float(value.detach()), (kind, value_o, float(value.detach()))
        assert np.array_equal(grad_o.astype(np.float32), f.grad.numpy()[0, 0]), kind
        value64, grad64 = cases.sparse_oracle(flux, kind, x0, y0, dtype=np.float64)
        assert abs(value64 - value_o) <= 1e-5 * abs(value64) and cases.rel_linf(grad_o, grad64) < 1e-5
        out[f"{kind}/offsets"] = np.array([x0, y0], dtype=np.float64)
        out[f"{kind}/value"] = np.float64(value.detach())
        out[f"{kind}/grad"] = f.grad.numpy()[0, 0]
        print("priors", kind, "ok", (x0, y0), float(value.detach()))

    for width in cases.SMOOTH_WIDTHS:
        prior = SmoothnessPrior(width=width)
        kernel = prior.kernel.numpy()[0, 0]
        assert np.array_equal(kernel, cases.gaussian_kernel(width)) and kernel.dtype == np.float64
        f = image.clone().requires_grad_(True)
        value = prior(f)
        value.backward()
        fo = image.clone().requires_grad_(True)
        value_o = cases.SmoothnessPriorRef(width)(fo)
        value_o.backward()
        assert float(value_o.detach()) == float(value.detach()) and np.array_equal(fo.grad.numpy(), f.grad.numpy())
        value64, grad64 = cases.smoothness_oracle(flux, kernel, np.float64)
        assert abs(value64 - float(value.detach())) <= 1e-6 * abs(value64), (value64, float(value.detach()))
        assert cases.rel_linf(f.grad.numpy()[0, 0], grad64) < 1e-6
        tag = f"smooth/{width}"
        out[f"{tag}/kernel"] = kernel
        out[f"{tag}/value"] = np.float64(value.detach())
        out[f"{tag}/grad"] = f.grad.numpy()[0, 0]
        print("priors", tag, "ok", kernel.shape, float(value.detach()))

    # the fits: 32 x 32 scene, two observations, default generators
    for tag, make_ref, make_oracle in (
        ("fit_subpix", lambda: InverseGammaPrior(cycle_spin_subpix=True), lambda: cases.SubpixPriorRef("inverse-gamma")),
        ("fit_smooth", lambda: SmoothnessPrior(), lambda: cases.SmoothnessPriorRef()),
    ):
        rs = np.random.RandomState(cases.FIT_SEED)
        datasets = {f"o{i}": mg.scene(cases.FIT_SHAPE, mg.asym_psf((7, 7), 1.2 + 0.3 * i, 1.6), rs, n_points=4, bkg=0.8)
                    for i in range(2)}
        flux_init = rs.gamma(2, size=cases.FIT_SHAPE) * 0.5 + 0.1
        comp = SpatialFluxComponent.from_numpy(flux=flux_init, prior=make_ref())
        res = MAPDeconvolver(n_epochs=cases.FIT_EPOCHS, display_progress=False).run(datasets=datasets, components=comp)
        final, trace = cpu_ref.map_fit_sequential(datasets, {"flux": flux_init}, {"flux": make_oracle()},
                                                  n_epochs=cases.FIT_EPOCHS)
        assert np.array_equal(final["flux"], res.flux_total), np.abs(final["flux"] - res.flux_total).max()
        assert trace[-1]["total"] == res.trace_loss[-1]["total"]
        out.update({f"{tag}/{k}": v for k, v in mg.pack_datasets(datasets).items()})
        out.update({f"{tag}/flux_init": flux_init, f"{tag}/flux_final": res.flux_total})
        out.update({f"{tag}/{k}": v for k, v in mg.trace_to_arrays(res.trace_loss).items()})
        print("priors", tag, "ok", res.trace_loss[-1]["total"])

    path = REPO / "tests" / "golden" / "priors.npz"
    np.savez_compressed(path, **out)
    print(path.name, path.stat().st_size // 1024, "KiB")


if __name__ == "__main__":
    main()

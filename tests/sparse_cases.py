"""Shared by tests/test_sparse_component_golden.py (CPU), tests/test_gpu_sparse_component.py (GPU) and
tools/make_golden_sparse.py: the cases of the sparse point-source flux component, its CPU oracle in float32 / float64 (the
reference's torch operations; pinned against the live reference when the generator wrote tests/golden/sparse_component.npz)
and a sequential and a joint fit harness for a mixed component set, assembled from `oracle.cpu_ref` pieces.

Axes: as in the reference (`y, x = self.indices`, jolideco/models/core.py:198-223) ``x_pos`` runs along the first image axis
(rows) and ``y_pos`` along the second (columns)."""
import functools

import numpy as np
import torch

from oracle import cpu_ref
from prior_cases import bound, rel_linf  # noqa: F401  (the project's rule: 4 x the float32 oracle's own error, floor 1e-6)

# (a) the reference's own case (jolideco/models/tests/test_core.py:78-85)
CASE_A_SHAPE = (25, 25)
CASE_A = {"flux": [3.7, 2.1, 4.2], "x_pos": [7.2, 12.1, 19.2], "y_pos": [7.7, 3.1, 14.2]}
CASE_B_SHAPE = (12, 16)  # (not square: pins which coordinate runs along which axis)
UPSTREAM_SEED = 2207

# render / backward kernels: smaller than a block's sources | one row | one column | odd sizes | several 16-byte groups
RENDER_SHAPES = [(5, 7), (1, 40), (40, 1), (33, 65), (64, 96)]
SOURCE_SETS = ["a", "b", "one", "random", "clustered"]
N_MANY = 1000

FIT_SHAPE, FIT_EPOCHS, FIT_SEED = (32, 32), 6, 411
FIT_POINTS = 3
# start = true position + offset, about 0.7 pixels away; the last keeps its x (row) coordinate exactly integer
FIT_OFFSETS = [(0.5, -0.5), (-0.45, 0.55), (0.0, 0.7)]
FIT_FLUX_START = 150.0


def case_a(shape=CASE_A_SHAPE):
    """Fixture set (a), its positions scaled from 25 x 25 into `shape`."""
    x = np.array(CASE_A["x_pos"]) * shape[0] / CASE_A_SHAPE[0]
    y = np.array(CASE_A["y_pos"]) * shape[1] / CASE_A_SHAPE[1]
    return _f32(CASE_A["flux"], x, y)


def case_b(shape=CASE_B_SHAPE):
    """Collisions and edges, placed relative to `shape` = (H, W): two sources in one pixel cell | two more that share a
    single pixel | one on exactly integer coordinates | one half a pixel beyond the last column | one wholly outside."""
    H, W = shape
    r, c = (H - 1) // 2, (W - 1) // 2
    rows = [r + 0.3, r + 0.6, r - 1.75, r - 0.5, float(min(r + 2, H - 1)), r + 0.25, -3.0]
    cols = [c + 0.2, c + 0.7, c - 1.6, c - 0.25, float(max(c - 2, 0)), W - 0.5, W + 5.0]
    flux = [1.5, 0.8, 2.5, 3.25, 4.0, 0.6, 7.0]
    return _f32(flux, rows, cols)


def _f32(flux, x_pos, y_pos):
    return tuple(np.asarray(v, dtype=np.float32) for v in (flux, x_pos, y_pos))


def source_set(kind, shape):
    """(flux, x_pos, y_pos) float32 arrays of the source set `kind` on an image of `shape`."""
    H, W = shape
    rs = np.random.RandomState(97 + 131 * H + W)
    if kind == "a":
        return case_a(shape)
    if kind == "b":
        return case_b(shape)
    if kind == "one":
        return _f32([2.75], [0.4 * (H - 1) + 0.3], [0.6 * (W - 1) + 0.45])
    if kind == "random":  # coordinates in (-1.5, 0) and (size - 1, size + 0.5) included
        return _f32(rs.uniform(0.2, 5.0, N_MANY), rs.uniform(-1.5, H + 0.5, N_MANY), rs.uniform(-1.5, W + 0.5, N_MANY))
    if kind == "clustered":  # all inside one 8 x 8 pixel window: dozens of sources on every pixel of it
        r0, c0 = max(0, min(3, H - 8)), max(0, min(5, W - 8))
        return _f32(rs.uniform(0.2, 5.0, N_MANY), rs.uniform(r0, r0 + 7.0, N_MANY), rs.uniform(c0, c0 + 7.0, N_MANY))
    raise ValueError(kind)


def upstream(shape, seed=UPSTREAM_SEED):
    """Seeded d loss / d image."""
    return np.random.RandomState(seed + 7 * shape[0] + shape[1]).normal(size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ oracle
def grid_weights(x, y, x0, y0):
    """jolideco/utils/torch.py:31-38, operation by operation."""
    dx = torch.abs(x - x0)
    dx = torch.where(dx < 1, 1 - dx, 0)
    dy = torch.abs(y - y0)
    dy = torch.where(dy < 1, 1 - dy, 0)
    return dx * dy


def render(param, x_pos, y_pos, shape, use_log_flux=True):
    """`SparseSpatialFluxComponent.flux` (jolideco/models/core.py:198-232) on tensors of one dtype -> (1, 1, H, W)."""
    dtype = param.dtype
    idx = torch.arange(shape[1], dtype=torch.float32).to(dtype).reshape(1, 1, 1, 1, -1)
    idy = torch.arange(shape[0], dtype=torch.float32).to(dtype).reshape(1, 1, 1, -1, 1)
    y, x = idx, idy  # (the reference's `y, x = self.indices`)
    weights = grid_weights(x=x, y=y, x0=x_pos.reshape(-1, 1, 1, 1, 1), y0=y_pos.reshape(-1, 1, 1, 1, 1))
    flux = torch.exp(param) if use_log_flux else param
    return (weights * flux.reshape(-1, 1, 1, 1, 1)).sum(axis=0)


def parameter(flux, use_log_flux=True):
    """The float32 parameter vector of the component for linear fluxes `flux` (its constructor's operations)."""
    flux = torch.from_numpy(np.asarray(flux, dtype=np.float32))
    return (torch.log(flux) if use_log_flux else flux).numpy()


def oracle(param, x_pos, y_pos, shape, use_log_flux=True, grad_image=None, dtype=np.float64):
    """(image, (grad_param, grad_x, grad_y)) in `dtype` for the FLOAT32 values `param`, `x_pos`, `y_pos`; gradients of
    sum(grad_image * image) by autograd (None without `grad_image`)."""
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    leaves = [torch.tensor(np.asarray(v, dtype=np.float32)).to(tdtype).requires_grad_(True) for v in (param, x_pos, y_pos)]
    image = render(*leaves, shape, use_log_flux)
    grads = None
    if grad_image is not None:
        (image[0, 0] * torch.tensor(np.asarray(grad_image, dtype=np.float32)).to(tdtype)).sum().backward()
        grads = tuple(leaf.grad.numpy().astype(np.float64) for leaf in leaves)
    return image.detach().numpy()[0, 0], grads


@functools.lru_cache(maxsize=None)
def cached_oracle(kind, shape, use_log_flux, dtype_name):
    flux, x_pos, y_pos = source_set(kind, shape)
    return oracle(parameter(flux, use_log_flux), x_pos, y_pos, shape, use_log_flux, upstream(shape),
                  np.dtype(dtype_name).type)


# --------------------------------------------------------------------------------------------------------- fit harness
def fit_scene(seed=FIT_SEED, shape=FIT_SHAPE, n_points=FIT_POINTS, scene=None, asym_psf=None):
    """The datasets of fixture (c) -- two observations of ONE scene through different PSFs -- and the true source
    positions (rows, columns).  `scene` / `asym_psf`: the generator's functions (oracle/refload/make_golden.py)."""
    datasets, truth = {}, None
    for i in range(2):
        rs = np.random.RandomState(seed)  # (the same points in both observations)
        replay = np.random.RandomState(seed)
        datasets[f"o{i}"] = scene(shape, asym_psf((7, 7), 1.2 + 0.3 * i, 1.6), rs, n_points=n_points, bkg=0.8)
        truth = [(replay.randint(0, shape[0]), replay.randint(0, shape[1]), replay.uniform(100, 800)) for _ in range(n_points)]
    return datasets, truth


def fit_start(truth, shape=FIT_SHAPE, seed=FIT_SEED):
    """(diffuse flux_init, (flux, x_pos, y_pos)) the fits of fixture (c) start from."""
    rs = np.random.RandomState(seed + 1)
    flux_init = rs.gamma(2, size=shape) * 0.5 + 0.1
    rows = [np.clip(r + dr, 0.0, shape[0] - 1.0) for (r, _, _), (dr, _) in zip(truth, FIT_OFFSETS)]
    cols = [np.clip(c + dc, 0.25, shape[1] - 1.25) for (_, c, _), (_, dc) in zip(truth, FIT_OFFSETS)]
    return flux_init, _f32([FIT_FLUX_START] * len(truth), rows, cols)


def fit_harness(datasets, flux_init, sources, n_epochs, mode="sequential", priors=None, use_log_flux=True, beta=1.0,
                learning_rate=0.1, frozen=False, names=("diffuse", "points"), record_first_grads=False, optimizer="adam"):
    """The reference's fit of a dense component `names[0]` (from `flux_init`) and a sparse component `names[1]` (from
    `sources` = (flux, x_pos, y_pos)), in the working precision of `cpu_ref.precision`: ONE optimizer over all parameters;
    "sequential": one step per dataset on L_d - beta * logprior / n_datasets and a trace row on the fluxes of the last step
    (jolideco/core.py:209-247); "joint": one step per epoch on the summed objective, the trace row from that step's forward
    pass (`cpu_ref.map_fit_joint`).  The sparse parameters start from their float32 values in every precision.
    Returns {"diffuse", "flux", "x_pos", "y_pos", "image", "trace"[, "first_grads"]}."""
    names_d = list(datasets)
    priors = priors or {}
    prior_list = [priors.get(name, cpu_ref.UniformPriorRef()) for name in names]
    theta = cpu_ref.log_flux_parameter(flux_init)
    working = theta.dtype
    shape = tuple(theta.shape[-2:])
    flux, x_pos, y_pos = sources
    sparse = [torch.tensor(v).to(working).requires_grad_(not frozen)
              for v in (parameter(flux, use_log_flux), np.asarray(x_pos, np.float32), np.asarray(y_pos, np.float32))]
    data = [cpu_ref.DatasetRef.from_numpy(datasets[n], list(names)) for n in names_d]
    optimizer_cls = torch.optim.Adam if optimizer == "adam" else torch.optim.SGD  # (jolideco/core.py:41)
    optimizer = optimizer_cls([theta] + ([] if frozen else sparse), lr=learning_rate)
    trace, first_grads = [], None

    def fluxes_now():
        return cpu_ref.to_flux(theta), render(*sparse, shape, use_log_flux)

    for _ in range(n_epochs):
        if mode == "sequential":
            for d in data:
                optimizer.zero_grad()
                fluxes = fluxes_now()
                loss = d.loss(fluxes)
                loss_prior = sum(p(f) for f, p in zip(fluxes, prior_list))
                (loss - beta * loss_prior / len(data)).backward()
                if first_grads is None:
                    first_grads = [None if v.grad is None else v.grad.numpy().copy() for v in sparse]
                optimizer.step()
            with torch.no_grad():
                loss_datasets = [d.loss(fluxes).item() for d in data]
                loss_priors = [torch.as_tensor(p(f)).item() for f, p in zip(fluxes, prior_list)]
        else:
            optimizer.zero_grad()
            fluxes = fluxes_now()
            total, losses, values = cpu_ref.joint_loss(data, fluxes, prior_list, beta)
            total.backward()
            if first_grads is None:
                first_grads = [None if v.grad is None else v.grad.numpy().copy() for v in sparse]
            optimizer.step()
            loss_datasets = [v.item() for v in losses]
            loss_priors = [torch.as_tensor(v).item() for v in values]
        trace.append(cpu_ref._trace_row(names_d, list(names), loss_datasets, loss_priors, beta))
    with torch.no_grad():
        diffuse, image = fluxes_now()
        source_flux = torch.exp(sparse[0]) if use_log_flux else sparse[0]
    out = {"diffuse": diffuse.numpy()[0, 0], "image": image.numpy()[0, 0], "flux": source_flux.detach().numpy().copy(),
           "x_pos": sparse[1].detach().numpy().copy(), "y_pos": sparse[2].detach().numpy().copy(), "trace": trace}
    if record_first_grads:
        out["first_grads"] = first_grads
    return out


def fit_bounds(run32, run64, floor=1e-5):
    """Per quantity of the sparse component: (the float32 harness run's error against the float64 run) x 4, floor 1e-5,
    relative to the largest magnitude of the value (DESIGN_LOG.md section 5: the yardstick of a fit is the harness's own
    float32 error)."""
    return {key: max(4.0 * rel_linf(run32[key], run64[key]), floor) for key in ("flux", "x_pos", "y_pos")}

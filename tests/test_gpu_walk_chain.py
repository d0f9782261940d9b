"""The chained plain strip walk (csrc/walkconv.hip, option JD_SEP_WALK_CHAIN = 2 .. 4): a block is a chain of waves on
vertically adjacent tiles of one strip, and a wave with a lower neighbour takes the row-pass results of its last 2 WH
rows from that neighbour's LDS stash instead of computing them.  The handed-over value is the one the wave would have
computed, so every launch must give the BITS of the one-wave-per-block kernels (JD_SEP_WALK_CHAIN = 1); the float64 oracle
of tests/step_oracle.py ties those bits to the truth (relative L-inf 1e-5 on images, 5e-6 on losses: the tolerances of the
joint-step tests of tests/test_gpu_baseline_parity.py).

Tile heights are forced to the smallest (38 rows in the 17-tap frame, 40 in the 33-tap frame); image heights are
38 k + r and 40 k + r for k = 1, 2, 4, 5: no chain, a chain of two, one full chain of four, a full chain with a chain of one
or two behind it.  With r = 3 the last tile is shorter than the 2 WH stashed rows.  Widths: one strip (72) and several strips
with a ragged last one (520).  The PSFs are Gaussians that are off centre in their arrays: a row offset of one shows."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_linf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHAINS = (2, 3, 4)
TILE = {17: 38, 33: 40}
HEIGHTS = {frame: [TILE[frame] * k + r for k in (1, 2, 4, 5) for r in (0, 3)] for frame in (17, 33)}
WIDTHS = (72, 520)
BATCH_HEIGHTS = tuple(sorted(set(HEIGHTS[17]) | set(HEIGHTS[33])))  # both tilings on one image: every height of either list
IMAGE_TOL, LOSS_TOL = 1e-5, 5e-6


def _psf(frame, index=0):
    """A separable Gaussian whose centre lies (dy, dx) pixels off the centre of its frame x frame array."""
    sigma, dy, dx = ((1.3 + 0.2 * index, 1.5, -1.0) if frame == 17 else (3.0 + 0.2 * index, 2.0, -1.5))
    t = np.arange(frame) - (frame - 1) / 2
    gy, gx = np.exp(-0.5 * ((t - dy) / sigma) ** 2), np.exp(-0.5 * ((t - dx) / sigma) ** 2)
    psf = np.outer(gy, gx)
    return (psf / psf.sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(H, W, n, seed=5):
    """flux, an image to convolve, and per dataset (exposure, background, counts, stirling) -- numpy, made once per shape"""
    from jolideco_amd.ops import stirling_mean

    rs = np.random.RandomState(seed + 1000 * H + W)
    flux = rs.gamma(5.0, size=(H, W)).astype(np.float32)
    image = rs.normal(size=(H, W)).astype(np.float32)
    data = []
    for i in range(n):
        exposure = ((1.0 + 0.1 * i) * (1.0 + 0.4 * np.linspace(-1, 1, H)[:, None] * np.ones((H, W)))).astype(np.float32)
        counts = rs.poisson(5.0, size=(H, W)).astype(np.float32)
        data.append((exposure, np.full((H, W), 0.5 + 0.1 * i, dtype=np.float32), counts, stirling_mean(counts)))
    return flux, image, tuple(data)


@functools.lru_cache(maxsize=None)
def _oracle_step(H, W, frames):
    """float64 step of every dataset: (sum of the gradients, [gradient per dataset], [npred], [loss])"""
    from step_oracle import step_oracle

    flux, _, data = _inputs(H, W, len(frames))
    outs = [step_oracle(flux, d[0], _psf(f, i), d[1], d[2], 1) for i, (f, d) in enumerate(zip(frames, data))]
    grads = [o["grad_flux"] for o in outs]
    return sum(grads), grads, [o["npred"] for o in outs], [o["loss"] for o in outs]


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _plan(H, W, frames, size):
    """A separable plan of size x size taps and the operators of the datasets' PSFs (17-tap ones embedded in zeros)."""
    from jolideco_amd.models.npred import embed_kernel
    from jolideco_amd.ops import ConvPlan

    plan = ConvPlan(H, W, size, size, DEV, method="separable")
    khats = []
    for i, frame in enumerate(frames):
        psf = _psf(frame, i)
        khats.append(plan.psf_spectrum(_to_dev(psf if frame == size else embed_kernel(psf, (size, size)))))
        assert plan.walk_frame(khats[-1]) == frame
    return plan, khats


def _force_tiles(jd_option, cols=None):
    jd_option("JD_SEP_WALK", 1)
    for key in ("JD_SEP_WALK_ROWS", "JD_SEP_WALK_ADJ_ROWS"):
        jd_option(key, TILE[17])
    for key in ("JD_SEP_WALK_ROWS33", "JD_SEP_WALK_ADJ_ROWS33"):
        jd_option(key, TILE[33])
    jd_option("JD_SEP_WALK_COLS", cols)
    jd_option("JD_SEP_WALK_ADJ_COLS", cols)


def _assert_bits(new, old, what):
    for name in old:
        assert torch.equal(new[name], old[name]), f"{what}: {name} differs from the unchained launch"


def _columns(frame):
    return (2, 4) if frame == 17 else (None,)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("frame,H", [(f, h) for f in (17, 33) for h in HEIGHTS[f]])
def test_forward_poisson_of_one_dataset(jd_option, frame, H, W):
    """jd_npred_poisson_fwd_bwd of one dataset: the chained forward + Poisson launch and the chained plain adjoint behind
    it.  Gradient (written, and accumulated into a non-zero image), npred and the loss."""
    flux, _, data = _inputs(H, W, 1)
    plan, (khat,) = _plan(H, W, (frame,), frame)
    exposure, background, counts = (_to_dev(a) for a in data[0][:3])
    flux_d = _to_dev(flux)

    def step():
        out = {}
        for name, accumulate in (("grad", False), ("grad+=", True)):  # (+=: into a non-zero image)
            loss, grad, npred = torch.zeros(1, device=DEV), torch.full((H, W), 0.25, device=DEV), torch.empty((H, W), device=DEV)
            plan.npred_poisson_fwd_bwd([flux_d], [exposure], [khat], background, counts, data[0][3], loss, grads=[grad],
                                       accumulate=accumulate, npred_out=npred)
            out.update({name: grad, "npred": npred, "loss": loss})
        torch.cuda.synchronize()
        assert not torch.equal(out["grad"], out["grad+="])
        return out

    grad_o, _, npred_o, loss_o = _oracle_step(H, W, (frame,))
    for cols in _columns(frame):
        _force_tiles(jd_option, cols)
        if frame == 33:  # (a launch of one frame takes its tile height from the plain options)
            jd_option("JD_SEP_WALK_ROWS", TILE[33])
            jd_option("JD_SEP_WALK_ADJ_ROWS", TILE[33])
        jd_option("JD_SEP_WALK_CHAIN", 1)
        old = step()
        for chain in CHAINS:
            jd_option("JD_SEP_WALK_CHAIN", chain)
            _assert_bits(step(), old, f"columns {cols}, chain {chain}")
        errs = (rel_linf(old["grad"].cpu().numpy(), grad_o), rel_linf(old["npred"].cpu().numpy(), npred_o[0]),
                abs(float(old["loss"]) / loss_o[0] - 1))
        print(f"columns {cols}: gradient {errs[0]:.2e}, npred {errs[1]:.2e}, loss {errs[2]:.1e}")
        assert errs[0] < IMAGE_TOL and errs[1] < IMAGE_TOL and errs[2] < LOSS_TOL
    plan.close()


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("frame,H", [(f, h) for f in (17, 33) for h in HEIGHTS[f]])
def test_plain_convolution_and_adjoint(jd_option, frame, H, W):
    """jd_conv_same and jd_conv_same_adjoint (without and with accumulate) through the chained plain walk."""
    from step_oracle import conv_same

    _, image, data = _inputs(H, W, 1)
    plan, (khat,) = _plan(H, W, (frame,), frame)
    image_d, scale = _to_dev(image), _to_dev(data[0][0])

    def calls():
        out = {"conv": plan.conv_same(image_d, scale, khat), "adjoint": plan.conv_same_adjoint(image_d, scale, khat)}
        out["adjoint+="] = plan.conv_same_adjoint(image_d, scale, khat, grad_image=torch.full((H, W), 0.25, device=DEV),
                                                  accumulate=True)
        torch.cuda.synchronize()
        return out

    x = torch.tensor(image.astype(np.float64) * data[0][0], requires_grad=True)
    psf = torch.tensor(_psf(frame).astype(np.float64))
    conv_o = conv_same(x, psf, "direct")
    g = torch.tensor(image.astype(np.float64), requires_grad=True)  # adjoint: d/dg' of <conv(g' * scale), image> at any g'
    (conv_same(g * torch.tensor(data[0][0].astype(np.float64)), psf, "direct") * torch.tensor(image.astype(np.float64))).sum().backward()
    conv_o, adj_o = conv_o.detach().numpy(), g.grad.numpy()
    for cols in _columns(frame):
        _force_tiles(jd_option, cols)
        if frame == 33:
            jd_option("JD_SEP_WALK_ROWS", TILE[33])
            jd_option("JD_SEP_WALK_ADJ_ROWS", TILE[33])
        jd_option("JD_SEP_WALK_CHAIN", 1)
        old = calls()
        for chain in CHAINS:
            jd_option("JD_SEP_WALK_CHAIN", chain)
            _assert_bits(calls(), old, f"columns {cols}, chain {chain}")
        errs = (rel_linf(old["conv"].cpu().numpy(), conv_o), rel_linf(old["adjoint"].cpu().numpy(), adj_o),
                rel_linf(old["adjoint+="].cpu().numpy(), 0.25 + adj_o))
        print(f"columns {cols}: conv {errs[0]:.2e}, adjoint {errs[1]:.2e}, accumulated adjoint {errs[2]:.2e}")
        assert max(errs) < IMAGE_TOL
    plan.close()


FRAMES = (17, 17, 33)


def _batch(H, W):
    flux, _, data = _inputs(H, W, len(FRAMES))
    plan, khats = _plan(H, W, FRAMES, 33)
    dev = [tuple(_to_dev(a) for a in d[:3]) + (d[3],) for d in data]
    return plan, khats, dev, _to_dev(flux)


def _library_step(plan, khats, data, flux, addends=None, side_stream=None):
    losses = [torch.zeros(1, device=DEV) for _ in data]
    grad = torch.full(flux.shape, 0.25, device=DEV)  # (overwritten: accumulate = False)
    used = plan.npred_poisson_batch_fwd_bwd(flux, [d[0] for d in data], khats, [d[1] for d in data], [d[2] for d in data],
                                            [d[3] for d in data], losses, grad=grad, addends=addends, side_stream=side_stream)
    torch.cuda.synchronize()
    return grad, torch.cat(losses), used


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", BATCH_HEIGHTS)
def test_batched_forward_launch_over_both_frames(jd_option, H, W):
    """The joint step of 2 + 1 datasets: the chained launch of both tilings (walk_mixed_chain_kernel), then the exchange
    launch of the 17-tap adjoints (not chained) and the plain accumulating walk of the one 33-tap adjoint (chained)."""
    plan, khats, data, flux = _batch(H, W)
    grad_o, _, _, losses_o = _oracle_step(H, W, FRAMES)
    for cols in (2, 4):
        _force_tiles(jd_option, cols)
        jd_option("JD_SEP_WALK_CHAIN", 1)
        grad, losses, _ = _library_step(plan, khats, data, flux)
        for chain in CHAINS:
            jd_option("JD_SEP_WALK_CHAIN", chain)
            grad_c, losses_c, _ = _library_step(plan, khats, data, flux)
            assert torch.equal(grad_c, grad) and torch.equal(losses_c, losses), f"columns {cols}, chain {chain}"
        err_g, err_l = rel_linf(grad.cpu().numpy(), grad_o), np.max(np.abs(losses.cpu().numpy() / np.array(losses_o) - 1))
        print(f"columns {cols}: gradient {err_g:.2e}, losses {err_l:.1e}")
        assert err_g < IMAGE_TOL and err_l < LOSS_TOL
    plan.close()


@pytest.mark.parametrize("beside", [True, False], ids=["second-stream", "one-stream"])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", BATCH_HEIGHTS)
def test_addend_launch(jd_option, H, W, beside):
    """The addend form of the library's step (tests/test_gpu_adjoint_addends.py): the 33-tap adjoint goes to an image of its
    own through the plain walk over a dataset table.  Gradient image, addend image and losses; the oracle sees their sum."""
    plan, khats, data, flux = _batch(H, W)
    grad_o, grads_o, _, losses_o = _oracle_step(H, W, FRAMES)
    _force_tiles(jd_option, 4)

    def step():
        addends = [torch.full((H, W), -7.0, device=DEV) for _ in range(2)]
        grad, losses, used = _library_step(plan, khats, data, flux, addends=addends,
                                           side_stream=torch.cuda.Stream(device=DEV) if beside else None)
        assert used == 1 and bool((addends[1] == -7.0).all())
        return {"grad": grad, "addend": addends[0], "losses": losses}

    jd_option("JD_SEP_WALK_CHAIN", 1)
    old = step()
    for chain in CHAINS:
        jd_option("JD_SEP_WALK_CHAIN", chain)
        _assert_bits(step(), old, f"chain {chain}")
    errs = (rel_linf((old["grad"] + old["addend"]).cpu().numpy(), grad_o), rel_linf(old["addend"].cpu().numpy(), grads_o[2]),
            np.max(np.abs(old["losses"].cpu().numpy() / np.array(losses_o) - 1)))
    print(f"gradient {errs[0]:.2e}, addend {errs[1]:.2e}, losses {errs[2]:.1e}")
    assert errs[0] < IMAGE_TOL and errs[1] < IMAGE_TOL and errs[2] < LOSS_TOL
    plan.close()

"""Recording stand-ins for `FitSession`'s epoch body: a session made of `FitSession.__new__` plus attributes, CPU tensors,
a recording Poisson loss, recording priors, a recording `DistContext`, a recording optimizer step -- no library.  An epoch
run on them leaves the ordered list of the calls it made.  `tools/make_golden_epoch_sequences.py` wrote the lists of the
body this one replaced to tests/golden/epoch_sequences.json; tests/test_epoch_sequence.py holds the present body to them.

Everything takes the `jolideco_amd.core` MODULE to work on, so that the tool can run another checkout's."""
import contextlib
import types

import torch

N_EPOCHS = 3


class Names:
    """Names of tensors by the storage they view: ``base[offset:offset + numel]``."""

    def __init__(self):
        self.bases = []

    def add(self, name, tensor):
        self.bases.append((name, tensor.data_ptr(), tensor.numel() * tensor.element_size()))
        return tensor

    def __call__(self, t):
        if t is None:
            return None
        if isinstance(t, (list, tuple)):
            return [self(x) for x in t]
        p = t.data_ptr()
        for name, begin, size in self.bases:
            if begin <= p < begin + size:
                offset = (p - begin) // t.element_size()
                return f"{name}[{offset}:{offset + t.numel()}]"
        return "(a tensor of the call's own)"


def _plain(shifts):
    if shifts is None:
        return None
    return [float(v) if isinstance(v, float) else int(v) for v in shifts]


class RecPrior:
    """A prior that records its evaluations.  ``generator``: (name, torch.Generator) -- every evaluation draws a pair from
    it unless the shifts are passed in; None: a prior that draws nothing and has no `draw_shifts`."""

    def __init__(self, rec, ci, generator=None, fused=False, shardable=False, stride=4):
        self.rec, self.ci, self.shardable, self.stride = rec, ci, shardable, stride
        self.supports_fused_step = fused
        self.supports_phases = fused
        self.last_shifts = None
        if generator is not None:
            self.generator_name, self.generator = generator
            self.draw_shifts = self._draw_shifts

    def _draw_shifts(self):
        self.rec.draws[self.generator_name] = self.rec.draws.get(self.generator_name, 0) + 1
        self.last_shifts = tuple(int(v) for v in torch.randint(-2, 3, (2,), generator=self.generator))
        return self.last_shifts

    def n_patch_rows(self, shape):
        return (shape[-2] - 8) // self.stride + 1

    def _shifts(self, shifts):
        if isinstance(shifts, str):
            return self.draw_shifts() if hasattr(self, "draw_shifts") else None
        return getattr(shifts, "host", shifts)

    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, patch_rows=None, shifts="draw", band_out=None, phases=3):
        name = self.rec.names
        self.rec.log.append({
            "kind": "prior", "ci": self.ci, "flux": name(flux), "value": name(value_out), "grad": name(grad), "coef": coef,
            "shifts": _plain(self._shifts(shifts)), "phases": phases, "patch_rows": None if patch_rows is None else list(patch_rows),
            "band_out": None if band_out is None else band_out.numel(),
        })

    def device_fwd_bwd_step(self, flux, value_out, coef, step, shifts="draw", phases=3):
        name = self.rec.names
        self.rec.log.append({
            "kind": "prior+step", "ci": self.ci, "flux": name(flux), "value": name(value_out), "coef": coef,
            "shifts": _plain(self._shifts(shifts)), "phases": phases, "step": self.rec.step_args(step),
        })


class RecUniform:
    """The uniform prior: its evaluation is the fill of the value slot."""

    value_is_zero = True
    shardable = False

    def __init__(self, rec, ci):
        self.rec, self.ci = rec, ci

    def device_fwd_bwd(self, flux, value_out, grad=None, coef=0.0, patch_rows=None):
        self.rec.log.append({"kind": "uniform-fill", "ci": self.ci, "value": self.rec.names(value_out)})


class RecState:
    def __init__(self, rec, ci, shape, grad, frozen=False):
        names = rec.names
        self.name, self.shape, self.frozen = f"c{ci}", shape, frozen
        self.theta = names.add(f"theta{ci}", torch.zeros(shape))
        self.flux = [names.add(f"flux{ci}.{k}", torch.zeros(shape)) for k in range(2)]
        self.exp_avg = names.add(f"exp_avg{ci}", torch.zeros(shape))
        self.exp_avg_sq = names.add(f"exp_avg_sq{ci}", torch.zeros(shape))
        self.grad = grad.reshape(shape)
        self.cur, self.mask, self.use_log_flux, self.trace_sees_current = 0, None, True, False

    flux_cur = property(lambda self: self.flux[self.cur])
    flux_prev = property(lambda self: self.flux[1 - self.cur])
    flux_trace = property(lambda self: self.flux_cur if self.trace_sees_current else self.flux_prev)


class RecPoisson:
    """Records the likelihood calls.  A call that is given a gradient leaves one on the calibration parameters of its
    datasets, except on those in ``no_grad`` (a shift that is exactly zero never receives one)."""

    def __init__(self, rec, kind, params, no_grad=()):
        self.rec, self.kind, self.params, self.no_grad = rec, kind, params, set(no_grad)

    def _leave_gradients(self, indices):
        for li in indices:
            for p in self.params.get(li, ()):
                if id(p) not in self.no_grad:
                    p.grad = torch.zeros_like(p.data)

    def fwd_bwd(self, idx, fluxes, loss_out, grads=None, accumulate=False, flux_nonneg=False):
        name = self.rec.names
        self.rec.log.append({"kind": self.kind, "datasets": [idx], "fluxes": name(fluxes), "loss": name(loss_out),
                             "grads": name(grads), "accumulate": accumulate, "flux_nonneg": flux_nonneg})
        if grads is not None:
            self._leave_gradients([idx])

    def fwd_bwd_batch(self, indices, flux, loss_outs, grad=None, accumulate=False, flux_nonneg=False, addends=None, side_stream=None):
        name = self.rec.names
        self.rec.log.append({"kind": self.kind + "-batch", "datasets": list(indices), "fluxes": name(flux), "loss": name(loss_outs),
                             "grads": name(grad), "accumulate": accumulate, "flux_nonneg": flux_nonneg,
                             "addends": None if addends is None else len(addends), "side_stream": side_stream is not None})
        if grad is not None:
            self._leave_gradients(indices)
        return 0

    def fwd_bwd_batch_calibrated(self, indices, flux, loss_outs, grad=None, accumulate=False):
        name = self.rec.names
        self.rec.log.append({"kind": self.kind + "-batch-calibrated", "datasets": list(indices), "fluxes": name(flux),
                             "loss": name(loss_outs), "grads": name(grad), "accumulate": accumulate})
        if grad is not None:
            self._leave_gradients(indices)


class _Pending:
    def __init__(self, rec):
        self.rec = rec

    def wait(self):
        self.rec.log.append({"kind": "collective", "name": "wait"})


class Recorder:
    """The log of one session, the names of its tensors and the draw counts of its generators."""

    def __init__(self):
        self.log, self.names, self.draws = [], Names(), {}

    @staticmethod
    def step_args(args):
        return {"step_size": args.step_size, "bias2_sqrt": args.bias2_sqrt, "sgd": args.sgd, "bias_dev": bool(args.bias_dev),
                "addends": sum(1 for a in args.addend if a)}


def _make_dist(core, rec, rank, world_size, dry_run):
    class RecDist(core.DistContext):
        def all_reduce_sum(self, buffer):
            rec.log.append({"kind": "collective", "name": "all_reduce_sum", "buffer": rec.names(buffer)})
            return buffer

        def all_reduce_sum_async(self, buffer):
            rec.log.append({"kind": "collective", "name": "all_reduce_sum_async", "buffer": rec.names(buffer)})
            return None if self.dry_run else _Pending(rec)

        def all_gather_flat(self, out, piece):
            rec.log.append({"kind": "collective", "name": "all_gather_flat", "out": out.numel(), "piece": piece.numel()})
            return out

        def assert_same_on_all_ranks(self, values, what):
            pass

    return RecDist(rank, world_size, dry_run=dry_run)


# what a case may set (defaults below): the keys of CASES' dictionaries
DEFAULTS = dict(
    joint=True, components="mixed", n_datasets=3, batch=False, batch_calibrated=False, calibrated=(), optimizer="adam",
    no_grad=(), hook=False, n_val=0, world=None, overlap=True,
)

CASES = {
    # joint and sequential, batched and per-dataset likelihood; "mixed" components: a prior that fuses the step, a drawing
    # prior that does not and cannot be sharded (both on ONE generator), a frozen component, a uniform prior
    "joint-batched": dict(batch=True),
    "joint-per-dataset": dict(),
    "sequential-batched-trace": dict(joint=False, batch=True),
    "sequential-per-dataset": dict(joint=False),
    "joint-one-component-batched": dict(components="one", batch=True),
    # the batched calibrated route; calibration steppers with Adam and with SGD, one parameter without a gradient
    "joint-batched-calibrated-adam": dict(components="one", batch_calibrated=True, calibrated=(0, 2), no_grad=((2, 0),)),
    "joint-batched-calibrated-sgd": dict(components="one", batch_calibrated=True, calibrated=(0, 2), no_grad=((2, 0),),
                                         optimizer="sgd"),
    "joint-calibrated-adam": dict(calibrated=(0, 1, 2), no_grad=((1, 0),)),
    "joint-calibrated-sgd": dict(calibrated=(0, 2), no_grad=((0, 0),), optimizer="sgd"),
    "sequential-calibrated-adam": dict(joint=False, calibrated=(0, 2), no_grad=((2, 0),)),
    "sequential-calibrated-sgd": dict(joint=False, calibrated=(1, 2), no_grad=((1, 0),), optimizer="sgd"),
    # a replaced `_optimizer_step` (two arguments; no fused step)
    "joint-hook": dict(hook=True, batch=True),
    "sequential-hook": dict(joint=False, hook=True),
    # validation datasets
    "joint-validation": dict(n_val=2, batch=True),
    "sequential-validation": dict(joint=False, n_val=2, calibrated=(1,)),
    # sharded: (rank, world size, dry run, band plan); "sharded" components: two shardable priors (one image whose width is
    # no multiple of 4: its bands are added without the step), a non-shardable drawing prior, a frozen component, a uniform
    "sharded-bands-rank0": dict(components="sharded", world=(0, 2, False), calibrated=(0,)),
    "sharded-bands-rank1": dict(components="sharded", world=(1, 2, False), calibrated=(0,)),
    "sharded-bands-rank0-dry-run": dict(components="sharded", world=(0, 2, True)),
    "sharded-bands-rank1-dry-run": dict(components="sharded", world=(1, 2, True), batch=True),
    "sharded-no-bands-rank0": dict(components="sharded", world=(0, 2, False), overlap=False),
    "sharded-no-bands-rank1": dict(components="sharded", world=(1, 2, False), overlap=False, n_val=1),
    "sharded-bands-rank1-hook": dict(components="sharded", world=(1, 2, False), hook=True),
    "sharded-sequential-rank1": dict(joint=False, components="sharded", world=(1, 2, False)),
}


def build_session(core, case):
    """(session, recorder) of ``CASES[case]`` on the stand-ins."""
    opt = dict(DEFAULTS, **CASES[case])
    rec = Recorder()
    names = rec.names
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(4)
    if opt["components"] == "one":
        layout = [((24, 16), dict(generator=("g1", g1), fused=True, shardable=True), False)]
    elif opt["components"] == "mixed":
        layout = [((24, 16), dict(generator=("g1", g1), fused=True, shardable=True), False),
                  ((24, 16), dict(generator=("g1", g1)), False),
                  ((24, 16), dict(generator=("g2", g2), fused=True, shardable=True), True),
                  ((24, 16), "uniform", False),
                  ((24, 16), dict(), False)]
    else:
        layout = [((24, 16), dict(generator=("g1", g1), fused=True, shardable=True), False),
                  ((24, 16), dict(generator=("g1", g1)), False),
                  ((24, 18), dict(generator=("g1", g1), fused=True, shardable=True), False),
                  ((24, 16), dict(generator=("g2", g2), fused=True, shardable=True), True),
                  ((24, 16), "uniform", False)]

    def optimizer_step(states, step, stepped=None):
        # (`last_shifts`: what a replaced step that records the gradient reads as the shifts of ITS step)
        rec.log.append({"kind": "optimizer-step", "step": step, "stepped": None if stepped is None else sorted(stepped),
                        "last_shifts": [_plain(getattr(p, "last_shifts", None)) for p in s.priors]})
        for st in states:
            st.cur = 1 - st.cur

    Deconvolver = type("RecordingDeconvolver", (core.MAPDeconvolver,),
                       {"_optimizer_step": lambda self, states, step, stepped=(): optimizer_step(states, step, stepped)})
    cfg = Deconvolver(device="cuda", fit_mode="joint" if opt["joint"] else "sequential", optimizer_type=opt["optimizer"], beta=0.5)
    if opt["hook"]:
        cfg._optimizer_step = lambda states, step: optimizer_step(states, step)

    s = core.FitSession.__new__(core.FitSession)
    s.cfg, s.joint = cfg, opt["joint"]
    rank, world_size, dry_run = opt["world"] or (0, 1, False)
    s.dist = _make_dist(core, rec, rank, world_size, dry_run)
    n_all = opt["n_datasets"]
    # (a sharded joint fit: the datasets round-robin over the ranks; sequential mode runs full replicas)
    local = [d for d in range(n_all) if not (s.joint and s.dist.sharded) or d % world_size == rank]
    s.local_idx = [(d, i) for i, d in enumerate(local)]
    s.n_d, s.n_c, s.n_val = n_all, len(layout), opt["n_val"]
    numels = [h * w for (h, w), _, _ in layout]
    s.comm = names.add("comm", torch.zeros(sum(numels) + s.n_d + s.n_c + s.n_val))
    s.scalars = s.comm[sum(numels):]
    s.states, s.priors, offset = [], [], 0
    for ci, (shape, prior, frozen) in enumerate(layout):
        s.states.append(RecState(rec, ci, shape, s.comm[offset : offset + numels[ci]], frozen))
        s.priors.append(RecUniform(rec, ci) if prior == "uniform" else RecPrior(rec, ci, **prior))
        offset += numels[ci]

    params, no_grad, s.cal_optimizers = {}, [], []
    for i, d in enumerate(local):
        if d in opt["calibrated"]:
            params[i] = [torch.nn.Parameter(names.add(f"cal{d}.{k}", torch.zeros(n))) for k, n in enumerate((2, 1))]
            no_grad += [id(params[i][k]) for dd, k in opt["no_grad"] if dd == d]
            s.cal_optimizers.append(core._CalibrationStepper(params[i], cfg))
        else:
            s.cal_optimizers.append(None)
    poisson = RecPoisson(rec, "likelihood", params, no_grad)
    validation = RecPoisson(rec, "validation", {}) if s.n_val else None
    s.total_loss = types.SimpleNamespace(poisson_loss=poisson, poisson_loss_validation=validation, prior_weight=len(local))

    s.step, s.comm_events, s.prior_shares, s.has_sparse = 0, None, None, False
    s.fuse_optimizer_step = not opt["hook"]
    s.batch_joint = s.joint and opt["batch"]
    s.batch_joint_calibrated = s.joint and opt["batch_calibrated"]
    s.batch_trace = (not s.joint) and opt["batch"]
    s.flux_nonneg = True
    s.overlap_prior, s._side_stream = True, None
    s._addend_images, s._addend_stream, s.addends_used = None, None, 0
    s.step_scalars, s._graphs, s._epochs_done, s._total_epochs, s._planned_ok = None, {}, 0, 0, False
    s._timed = lambda name, fn: (rec.log.append({"kind": "timed", "name": name}), fn())[1]
    core.FitSession._setup_sharded_prior(s, opt["overlap"])
    if s.band_plan:
        names.add("band_send", s.band_send)
        names.add("band_recv", s.band_recv)
    return s, rec


@contextlib.contextmanager
def recording_library(core, rec):
    """The module-level calls of the epoch body -- the step of the small parameters, the band sums of `ops` -- replaced
    by recorders, and put back.  The step of the small parameters is one launch for Adam and for SGD; its log keeps the
    form of the recorded sequences: one entry with every stepped parameter for Adam, one entry per stepped parameter, in
    order, for SGD."""
    from importlib import import_module

    ops = import_module(core.__name__.rsplit(".", 1)[0] + ".ops")
    names = rec.names

    def step_parameters(cfg, items, cache, bias_dev=None):
        stepped = []
        for p, st in items:
            if p.grad is None:
                if bias_dev is not None:
                    raise RuntimeError("planned epoch: a calibration parameter lost its gradient between two epochs")
                continue
            st["step"] += 1
            stepped.append([names(p.data), st["step"]])
            if cfg.optimizer_type != "adam":
                rec.log.append({"kind": "sgd-step", "param": names(p.data), "grad": names(p.grad), "n": p.numel(),
                                "lr": cfg.optimizer_kwargs["lr"]})
        if cfg.optimizer_type == "adam":
            rec.log.append({"kind": "adam-step-many", "items": stepped, "bias_dev": bias_dev is not None})

    class Library:  # (no entry: a library call the epoch body makes on its own fails the case)
        pass

    def bands(grad, shifts, bands, chunk, y_ranges):
        rec.log.append({"kind": "add-rolled-bands", "grad": names(grad), "shifts": _plain(shifts), "bands": names(bands),
                        "chunk": chunk, "y_ranges": [list(r) for r in y_ranges]})

    def bands_step(shape, shifts, bands, chunk, y_ranges, step):
        rec.log.append({"kind": "add-rolled-bands+step", "shape": list(shape), "shifts": _plain(shifts), "bands": names(bands),
                        "chunk": chunk, "y_ranges": [list(r) for r in y_ranges], "step": rec.step_args(step)})

    patches = [(core, "_step_parameters", step_parameters), (core, "ptr", names), (core, "stream_ptr", lambda device=None: None),
               (core, "check", lambda status: None), (core._hip, "lib", lambda: Library),
               (ops, "add_rolled_bands", bands), (ops, "add_rolled_bands_step", bands_step)]
    saved = [(module, name, getattr(module, name)) for module, name, _ in patches]
    try:
        for module, name, value in patches:
            setattr(module, name, value)
        yield
    finally:
        for module, name, value in saved:
            setattr(module, name, value)


def run_case(core, case, epoch):
    """The log of N_EPOCHS epochs of ``CASES[case]``: ``epoch(session)`` enqueues one.  After each epoch an entry with the
    host state the epoch left: step count, buffer parity, the step counts of the calibration parameters, the last shifts
    of every prior and the draws made from every generator so far."""
    session, rec = build_session(core, case)
    with recording_library(core, rec):
        for _ in range(N_EPOCHS):
            epoch(session)
            rec.log.append({
                "kind": "epoch-end", "step": session.step, "cur": [st.cur for st in session.states],
                "calibration_steps": [None if opt is None else [st["step"] for st in opt.state] for opt in session.cal_optimizers],
                "last_shifts": [_plain(getattr(p, "last_shifts", None)) for p in session.priors], "draws": dict(sorted(rec.draws.items())),
            })
    return rec.log

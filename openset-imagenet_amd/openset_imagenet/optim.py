"""Fused optimizers over the flat parameter arena: one HIP launch per step instead of 162 x several.

Stand in for `torch.optim.Adam(params, lr)` / `torch.optim.SGD(params, lr, momentum=0.9)` built at reference
openset_imagenet/train.py:356-359 and stepped at train.py:139. They subclass torch.optim.Optimizer, keep per-parameter
state entries (`step`, `exp_avg`, `exp_avg_sq` / `momentum_buffer`) as VIEWS into flat state arenas, so `state_dict()` /
`load_state_dict()` round-trip with the stock torch optimizers and with the reference checkpoint dict
(`opt_state_dict`, train.py:54-60). `lr` and every other option are read from `param_groups` each step, so
`lr_scheduler.StepLR` and per-group schedules work.

Beyond the reference's call they take what a `torch.optim` user expects: any subset of ONE model's parameters, a list of group
dicts with per-group options, `add_param_group`, weight decay (L2 and decoupled: `AdamW`), AMSGrad, Nesterov momentum, dampening,
`maximize`, and torch's skipping rule for parameters with `requires_grad == False`. Whatever the layout, a step is one launch:
the plain `osi_adam_step` / `osi_sgd_step` when one group holds the whole arena with the reference's options (bit for bit the
launch of earlier releases), `osi_adam_step_groups` / `osi_sgd_step_groups` with a segment table otherwise.

`step(clip_norm=x, norm_type=2 | inf)` clips the gradient norm as `torch.nn.utils.clip_grad_norm_(params, x, norm_type)` followed by
`step()` would, without a host read: one streaming pass leaves the norm of `grad_scale * g` over the tensors this step updates and
the step's scalar `grad_scale * min(1, x / (norm + 1e-6))` in device memory (`osi_grad_clip_scale`, two launches), and the grouped
kernel reads that scalar there (`osi_*_step_groups_dev`). `opt.grad_norm` holds the pre-clip norm (a 0-dim device tensor), what
`clip_grad_norm_` returns; `clip_norm=float("inf")` only measures. The gradient arena itself is left as the backward wrote it: the
clipped gradients exist only inside the step. Without `clip_norm` a step is the launch it always was and `grad_norm` is None.
"""
import torch

from . import _native as N

_MAX_KERNEL_GROUPS = N.OPT_MAX_GROUPS
_MAX_SEGMENTS = N.OPT_MAX_SEGMENTS


def _arena_of(params):
    """The model that owns `params` in one flat arena (all parameters must come from one MI355X ResNet50)."""
    owner = None
    for p in params:
        o = getattr(p, "_osi_owner", None)
        o = o() if o is not None else None
        if o is None or (owner is not None and o is not owner):
            return None
        owner = o
    return owner


def _only_off(**flags):
    for k, v in flags.items():
        if v not in (None, False):
            raise ValueError(f"{k}={v!r}: the fused optimizers are their own implementation; pass None / False or use torch.optim.*")


def _check_clip(clip_norm, norm_type):
    """(max_norm, OSI_NORM_*) of step(clip_norm=, norm_type=); ValueError on anything clip_grad_norm_ would not make sense of"""
    if isinstance(clip_norm, bool) or not isinstance(clip_norm, (int, float)) or not clip_norm > 0:      # NaN fails the comparison
        raise ValueError(f"clip_norm must be a number > 0 (float('inf') measures only), got {clip_norm!r}")
    x = float(clip_norm)
    if isinstance(norm_type, bool) or not isinstance(norm_type, (int, float)) or norm_type not in (2, float("inf")):
        raise ValueError(f"norm_type must be 2 or float('inf'), got {norm_type!r}")
    return x, (N.NORM_L2 if norm_type == 2 else N.NORM_INF)


def split_decay(model, weight_decay, no_decay="norm_bias"):
    """The two-group ImageNet recipe: [{params with ndim > 1, weight_decay}, {BatchNorm weights and biases, linear biases,
    weight_decay 0}]. `model` may be a DistributedDataParallel wrapper."""
    if no_decay != "norm_bias":
        raise ValueError(f"split_decay: no_decay must be 'norm_bias', got {no_decay!r}")
    params = [p for p in getattr(model, "module", model).parameters()]
    return [dict(params=[p for p in params if p.ndim > 1], weight_decay=weight_decay),
            dict(params=[p for p in params if p.ndim <= 1], weight_decay=0.0)]


class _FlatOptimizer(torch.optim.Optimizer):
    _state_names = ()
    _has_step = True    # per-parameter "step" entry in the state dict (torch.optim.Adam has one, torch.optim.SGD does not)

    def __init__(self, model_or_params, defaults):
        self._model = None
        self._flat_state = {}
        self._pstep = {}             # arena index of a held parameter -> steps taken (torch's per-parameter `step`); read via _counts()
        self._lag = 0                # steps the parameters of the current table (_active) took since _pstep was last brought up to date
        self._active = ()
        self._version = 0            # bumped when the groups or the loaded state change: the cached table is rebuilt
        self._bound = -1             # the _version whose parameters have their state views bound
        self._plan = None
        self._held_cache = None
        self._spans = ()             # flat (begin, numel) pairs of the tensors of the current table: what a clipped step takes its norm over
        self._clip_buf = None        # (workspace, out2) of osi_grad_clip_scale, allocated once per device
        self.grad_norm = None        # the pre-clip norm of the latest step(clip_norm=...), a 0-dim device tensor; None otherwise
        if isinstance(model_or_params, torch.nn.Module):
            model_or_params = model_or_params.parameters()
        super().__init__(model_or_params, defaults)   # reference spelling: Adam(params=model.parameters(), lr=...)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)          # ValueError on a parameter that already sits in another group
        group = self.param_groups[-1]
        model = _arena_of(group["params"])
        if model is None or (self._model is not None and model is not self._model):
            self.param_groups.pop()
            raise ValueError("the fused optimizers step the flat arena of ONE MI355X ResNet50: every parameter must be one of that "
                             "model's own (model.parameters(), or a subset of them); use torch.optim.* for anything else")
        if self._model is None:
            self._model = model
            self._index = {id(p): i for i, p in enumerate(model._plist)}
        for p in group["params"]:
            self._pstep.setdefault(self._index[id(p)], 0)
        self._version += 1

    def _counts(self):
        """The per-parameter step counts, up to date. While one table is in use its parameters move together, so step() counts
        once (_lag) and the counts are folded into _pstep only when somebody reads them or the table changes."""
        if self._lag:
            ps = self._pstep
            for idx, gi in self._active:
                ps[idx] += self._lag
            self._lag = 0
        return self._pstep

    # `_steps`: the step count of an optimizer whose parameters all move together (what the plain launch takes)
    @property
    def _steps(self):
        return max(self._counts().values(), default=0)

    def _held(self):
        """[(user group index, arena index, parameter)] in group order."""
        if self._held_cache is None or self._held_cache[0] != self._version:
            held = [(gi, self._index[id(p)], p) for gi, g in enumerate(self.param_groups) for p in g["params"]]
            self._held_cache = (self._version, held, [p for _, _, p in held])
        return self._held_cache[1]

    def _wants(self, name, group):
        """Does a parameter of `group` carry the state tensor `name`?"""
        return True

    def _ensure_state(self):
        flat = self._model.flat_parameters()
        if self._bound == self._version and all(t.device == flat.device for t in self._flat_state.values()):
            return
        # the groups changed (add_param_group after a step, amsgrad switched on for a new group) or the model moved: allocate
        # what is missing and bind the views of every held parameter again
        names = [k for k in self._state_names if any(self._wants(k, g) for g in self.param_groups)]
        for k in names:
            old = self._flat_state.get(k)
            if old is None or old.device != flat.device:
                t = torch.zeros_like(flat)
                if old is not None:
                    t.copy_(old)
                self._flat_state[k] = t
        self._bind_views()

    def _bind_views(self):
        m = self._model
        counts = self._counts()
        self._bound = self._version
        for gi, idx, p in self._held():
            name, off, numel, shape = m._pinfo[idx]
            st = self.state[p]
            if self._has_step:
                st["step"] = torch.tensor(float(counts[idx]))
            for k in self._state_names:
                if k in self._flat_state and self._wants(k, self.param_groups[gi]):
                    st[k] = m._view(self._flat_state[k], off, numel, shape)

    def zero_grad(self, set_to_none=True):
        # the executor overwrites the whole gradient arena each backward; dropping the references is enough
        super().zero_grad(set_to_none=set_to_none)
        self._model._grads_fresh = False

    def _skip_step(self):
        """torch skips parameters whose .grad is None; here the arena is all-or-nothing: without a backward since the last
        zero_grad() there is nothing to apply (stepping would re-apply stale gradients). Frozen parameters are skipped one by
        one in the table (_plan_for)."""
        return not getattr(self._model, "_grads_fresh", False)

    # ---- which launch, which table -----------------------------------------------------------------------
    def _class_of(self, idx, group):
        """Parameters of one user group share a kernel group while this value is equal."""
        return self._pstep[idx]      # called from _plan_for, after _counts()

    def _plain_options(self, group):
        raise NotImplementedError

    def _plan_for(self):
        """(plain, segments, kernel groups): `plain` = one group holds the whole arena, everything requires grad and moves in
        step, so the plain launch applies if the options allow; `segments` = flat (begin4, end4, kernel group) triples, adjacent
        tensors of one kernel group merged; kernel groups = [(user group index, arena index of a representative parameter)].
        Rebuilt only when the groups, the requires_grad flags or a loaded state change: stepping the same set again keeps every
        class together."""
        held = self._held()
        flags = tuple([p.requires_grad for p in self._held_cache[2]])
        key = (self._version, flags)
        if self._plan is not None and self._plan[0] == key:
            return self._plan[1:]
        m = self._model
        self._counts()      # the counts of the table that goes away, before _active changes
        active = sorted((idx, gi) for (gi, idx, p), on in zip(held, flags) if on)
        kgroups, kindex, segments, spans = [], {}, [], []
        for idx, gi in active:
            k = (gi, self._class_of(idx, self.param_groups[gi]))
            if k not in kindex:
                kindex[k] = len(kgroups)
                kgroups.append((gi, idx))
            name, off, numel, shape = m._pinfo[idx]
            b4, e4, kg = off // 4, (off + numel + 3) // 4, kindex[k]
            if spans and spans[-2] + spans[-1] == off:   # the tensor before ends here, on a unit boundary: no alignment lanes between
                spans[-1] += numel
            else:
                spans += [off, numel]
            if segments and segments[-1][2] == kg and segments[-1][1] == b4:
                segments[-1][1] = e4
            else:
                segments.append([b4, e4, kg])
        if len(kgroups) > _MAX_KERNEL_GROUPS or len(segments) > _MAX_SEGMENTS:
            raise ValueError(f"the fused optimizers take at most {_MAX_KERNEL_GROUPS} distinct (parameter group, step count) pairs and "
                             f"{_MAX_SEGMENTS} arena segments per launch, got {len(kgroups)} and {len(segments)}: use torch.optim.* "
                             "for this layout")
        plain = len(self.param_groups) == 1 and len(active) == len(m._plist) == len(held) and len(kgroups) == 1
        self._plan = (key, plain, [v for s in segments for v in s], kgroups)
        self._active = active
        self._spans = spans
        return self._plan[1:]

    def _clip_scalar(self, grads, grad_scale, max_norm, norm):
        """Launch the norm over this step's tensors; returns the step's scalar (one device float) and sets grad_norm. No host read."""
        buf = self._clip_buf
        if buf is None or buf[1].device != grads.device:
            ws = torch.empty(max(int(N.lib().osi_grad_norm_workspace(grads.numel())), 16), dtype=torch.uint8, device=grads.device)
            buf = self._clip_buf = (ws, torch.zeros(2, device=grads.device))
        N.ops().grad_clip_scale(grads, self._spans, norm, float(grad_scale), max_norm, buf[0], buf[1])
        self.grad_norm = buf[1][0].clone()
        return buf[1][1:]

    def _stepped(self):
        """Count the step on every parameter that took part (those of the table: held and requiring grad)."""
        self._lag += 1

    # ---- state dict ----------------------------------------------------------------------------------------
    def state_dict(self):
        # torch's schema: entries only for parameters that have been stepped (or came in with a checkpoint)
        unstepped = {}
        counts = self._counts()
        if self._flat_state:
            self._ensure_state()   # parameters added since the last step: their views are bound before anybody looks
        for gi, idx, p in self._held():
            if p in self.state:
                if counts[idx] == 0:
                    unstepped[p] = self.state.pop(p)
                elif self._has_step:   # materialise torch's per-parameter step counters only when somebody looks
                    self.state[p]["step"] = torch.tensor(float(counts[idx]))
        try:
            return super().state_dict()
        finally:
            self.state.update(unstepped)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        m = self._model
        flat = m.flat_parameters()
        self._counts()
        self._flat_state = {}
        names = [k for k in self._state_names if any(self._wants(k, g) for g in self.param_groups)]
        for k in names:
            self._flat_state[k] = torch.zeros_like(flat)
        for gi, idx, p in self._held():
            name, off, numel, shape = m._pinfo[idx]
            st = self.state.get(p, {})
            self._pstep[idx] = self._loaded_steps(st)
            for k in names:
                if k in st and st[k] is not None:
                    m._view(self._flat_state[k], off, numel, shape).copy_(st[k])
        self._version += 1
        self._bind_views()

    def _loaded_steps(self, st):
        return int(float(st["step"])) if "step" in st else 0


def _check_adam(lr, betas, eps, weight_decay):
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


class Adam(_FlatOptimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad, maximize=, decoupled_weight_decay=) as one fused launch."""
    _state_names = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _check_adam(lr, betas, eps, weight_decay)
        _only_off(foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                     foreach=None, capturable=False, differentiable=False, fused=None,
                                     decoupled_weight_decay=decoupled_weight_decay))

    def _wants(self, name, group):
        return name != "max_exp_avg_sq" or bool(group.get("amsgrad", False))

    @staticmethod
    def _plain_options(g):
        return not (g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False))

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, clip_norm=None, norm_type=2.0):
        m = self._model
        self.grad_norm = None
        clip = None if clip_norm is None else _check_clip(clip_norm, norm_type)
        if self._skip_step():
            return
        plain, segments, kgroups = self._plan_for()
        if not kgroups:
            return
        self._ensure_state()
        p, gr = m.flat_parameters(), m.flat_gradients()
        fs = self._flat_state
        scalar = None if clip is None else self._clip_scalar(gr, grad_scale, *clip)
        if scalar is None and plain and self._plain_options(self.param_groups[0]):
            g = self.param_groups[0]
            N.ops().adam_step(p, gr, fs["exp_avg"], fs["exp_avg_sq"], float(g["lr"]), float(g["betas"][0]),
                              float(g["betas"][1]), float(g["eps"]), self._pstep[kgroups[0][1]] + self._lag + 1, float(grad_scale))
        else:
            rows = []
            for gi, idx in kgroups:
                g = self.param_groups[gi]
                rows += [float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g.get("weight_decay", 0)),
                         float(self._pstep[idx] + self._lag + 1), float(bool(g.get("decoupled_weight_decay", False))),
                         float(bool(g.get("amsgrad", False))), float(bool(g.get("maximize", False)))]
            if scalar is None:
                N.ops().adam_step_groups(p, gr, fs["exp_avg"], fs["exp_avg_sq"], fs.get("max_exp_avg_sq"), segments, rows, float(grad_scale))
            else:    # the same launch over the same table, the scalar read from device memory
                N.ops().adam_step_groups_dev(p, gr, fs["exp_avg"], fs["exp_avg_sq"], fs.get("max_exp_avg_sq"), segments, rows, scalar)
        self._stepped()


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay (p *= 1 - lr*weight_decay before the update), default 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)


class SGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov, maximize=) as one fused launch. A parameter of a group
    with momentum == 0 has `momentum_buffer: None` in the state dict and its slice of the buffer arena is never touched."""
    _state_names = ("momentum_buffer",)
    _has_step = False

    def __init__(self, params, lr=1e-3, momentum=0.9, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        _only_off(foreach=foreach, differentiable=differentiable, fused=fused)
        self._has_buf = {}    # arena index -> the momentum buffer holds a value (written by a step, or loaded): not torch's first step
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                     maximize=maximize, foreach=None, differentiable=False, fused=None))

    # torch initialises momentum_buffer = grad on the first step of a parameter whose buffer is None; a buffer that came in through
    # load_state_dict (own or stock torch.optim.SGD checkpoint, which carries no step counter) continues as mu*buf + g
    def _class_of(self, idx, group):
        return bool(self._has_buf.get(idx, False)) or not group["momentum"]

    @staticmethod
    def _plain_options(g):
        return not (g.get("weight_decay", 0) or g.get("dampening", 0) or g.get("nesterov", False) or g.get("maximize", False))

    def _plan_for(self):
        # a group whose momentum was switched on or off since the table was built changes its parameters' classes
        mom = tuple(bool(g["momentum"]) for g in self.param_groups)
        if getattr(self, "_mom", None) != mom:
            self._mom, self._plan = mom, None
        return super()._plan_for()

    def _loaded_steps(self, st):
        return 1 if st else 0

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for gi, idx, p in self._held():
            self._has_buf[idx] = self.state.get(p, {}).get("momentum_buffer") is not None

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, clip_norm=None, norm_type=2.0):
        m = self._model
        self.grad_norm = None
        clip = None if clip_norm is None else _check_clip(clip_norm, norm_type)
        if self._skip_step():
            return
        plain, segments, kgroups = self._plan_for()
        if not kgroups:
            return
        self._ensure_state()
        p, gr = m.flat_parameters(), m.flat_gradients()
        buf = self._flat_state["momentum_buffer"]
        scalar = None if clip is None else self._clip_scalar(gr, grad_scale, *clip)
        if scalar is None and plain and self._plain_options(self.param_groups[0]):
            # k_sgd writes the buffer whatever the momentum, so `first` is the first step of a fresh optimizer, momentum 0 included
            g = self.param_groups[0]
            started = plain_first = not self._has_buf.get(kgroups[0][1], False)
            N.ops().sgd_step(p, gr, buf, float(g["lr"]), float(g["momentum"]), bool(plain_first), float(grad_scale))
        else:
            rows, started, plain_first = [], False, False
            for gi, idx in kgroups:
                g = self.param_groups[gi]
                first = bool(g["momentum"]) and not self._has_buf.get(idx, False)   # a momentum == 0 group has no buffer to start
                started = started or first
                rows += [float(g["lr"]), float(g["momentum"]), float(g.get("dampening", 0)), float(g.get("weight_decay", 0)),
                         float(bool(g.get("nesterov", False))), float(first), float(bool(g.get("maximize", False)))]
            if scalar is None:
                N.ops().sgd_step_groups(p, gr, buf, segments, rows, float(grad_scale))
            else:
                N.ops().sgd_step_groups_dev(p, gr, buf, segments, rows, scalar)
        self._stepped()
        if started:
            for idx, gi in self._active:
                if plain_first or self.param_groups[gi]["momentum"]:
                    self._has_buf[idx] = True
            self._plan = None     # first-step parameters joined the others: the classes changed

    def state_dict(self):
        sd = super().state_dict()
        i = 0
        for gi, g in enumerate(self.param_groups):
            for q in g["params"]:
                if i in sd["state"] and not (g["momentum"] and self._has_buf.get(self._index[id(q)], False)):
                    sd["state"][i] = dict(sd["state"][i], momentum_buffer=None)
                i += 1
        return sd

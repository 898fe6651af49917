"""ResNet50 with the deep-feature and logits layers of the reference, executed by libosi_hip on an MI355X.

Drop-in for `openset_imagenet.model.ResNet50` (reference openset_imagenet/model.py:5-39):
same constructor `ResNet50(fc_layer_dim, out_features, logit_bias)`, `forward(image) -> (logits, features)`,
`model.logits.in_features / .out_features` (read at reference train.py:210-211) and the same 321 `state_dict()`
keys (`resnet_base.conv1.weight` ... `resnet_base.fc.bias`, `logits.weight`), so reference checkpoints load.

What is different underneath (nothing of torchvision / ATen / MIOpen runs):
  * all 162 parameter tensors are views into ONE flat fp32 arena (`_flat_params`), gradients into a second arena of the
    same layout (`_flat_grads`), BN running statistics into a third; conv weights keep the logical OIHW shape but are
    stored KRSC (= channels_last strides), which is what the implicit-GEMM kernels read directly;
  * `forward` is one C call (`osi_resnet50_forward`) that enqueues the whole network on the current HIP stream;
    `backward` is `osi_resnet50_backward`, run stage by stage so that a gradient all-reduce (dp.py) can start on the
    finished part of the arena while earlier layers are still being differentiated.
There is no CPU path: calling the module with a CPU tensor raises.
"""
import ctypes
import math
import os
import weakref

import torch
from torch import nn

from . import _native as N


class _Node(nn.Module):
    """Pure container mirroring one torchvision sub-module in the state_dict hierarchy (no forward of its own)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("sub-modules of the MI355X ResNet50 are parameter containers; call the model itself")


def debug_options_from_env():
    """Development A/B switches of the executor, read from the environment in ONE place and handed over explicitly through
    osi_resnet50_set_option (the library itself never reads the environment). Every default is the measured optimum; nothing here
    is needed to run the product. {option name: value} for the variables that are set:
        OSI_NO_OVERLAP=1      overlap 0           weight gradients stay on the main stream (serialised backward)
        OSI_FWD_FORK=0        fwd_fork 0          projection shortcut of the forward pass on the main stream
        OSI_SIDE_PRIO=n       side_priority_normal 1
        OSI_EVAL_FUSED=0      eval_fused 0        eval-mode forwards through the training topology on running statistics (no inference forms)
    (There is no switch for round 2's fused in-block activations: the unfused executor path no longer exists; its price on one box is the
    three-way A/B of the committed round-1 / round-2 / current trees, profiles/r03_ab_rounds.txt.)"""
    env = os.environ
    out = {}
    if env.get("OSI_NO_OVERLAP"):
        out["overlap"] = 0
    if env.get("OSI_FWD_FORK") == "0":
        out["fwd_fork"] = 0
    if env.get("OSI_SIDE_PRIO", "")[:1] == "n":
        out["side_priority_normal"] = 1
    if env.get("OSI_EVAL_FUSED") == "0":
        out["eval_fused"] = 0
    return out


class _Net:
    """Owner of one executor handle (fixed batch / image size)."""

    def __init__(self, B, H, W, F, O, logit_bias):
        self.h = ctypes.c_void_p()
        N.check(N.lib().osi_resnet50_create(ctypes.byref(self.h), B, H, W, F, O, int(bool(logit_bias))), "osi_resnet50_create")
        self.ws_bytes = N.lib().osi_resnet50_workspace_bytes(self.h)
        self.staged = False      # executor option "stage_join" = 0 has been set (data-parallel backward)
        self.trainable = None    # (unit mask, inference-form prefix units) last handed to osi_resnet50_set_trainable; None = the default
        self.owes_backward = False   # a differentiable forward ran and its backward has not finished
        for name, value in debug_options_from_env().items():
            N.check(N.lib().osi_resnet50_set_option(self.h, name.encode(), value), f"osi_resnet50_set_option({name})")

    def __del__(self):
        try:
            if self.h:
                N.lib().osi_resnet50_destroy(self.h)
                self.h = None
        except Exception:
            pass


class _BackboneFn(torch.autograd.Function):
    """Autograd node standing for the whole network: parameter gradients are written straight into the gradient arena; the
    gradient w.r.t. an NCHW `image` that requires grad is returned as that input's gradient. `anchor` stands for the parameters:
    a detached anchor (no parameter requires grad) makes the backward input-only (no parameter gradient is computed)."""

    @staticmethod
    def forward(ctx, image, anchor, model, flip, frozen=False):
        ctx.model = model
        ctx.set_materialize_grads(False)
        out = model._run_forward(image, True, flip, frozen)
        ctx.serial = model._fwd_serial
        return out

    @staticmethod
    def backward(ctx, dlogits, dfeatures):
        if ctx.serial != ctx.model._fwd_serial:
            raise RuntimeError("backward() of a forward pass that is no longer the model's latest one: the executor keeps the "
                               "activations of ONE forward (the reference loop is forward, loss, backward, step — train.py:132-139)")
        want_dx, want_params = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dimage = ctx.model._run_backward(dlogits, dfeatures, want_image=want_dx, param_grads=want_params)
        return dimage, None, None, None, None


class ResNet50(nn.Module):
    """Represents a ResNet50 model (reference model.py:5)."""

    def __init__(self, fc_layer_dim=1000, out_features=1000, logit_bias=True):
        super().__init__()
        self._F, self._O, self._logit_bias = int(fc_layer_dim), int(out_features), bool(logit_bias)
        lib = N.lib()
        probe = _Net(1, 32, 32, self._F, self._O, self._logit_bias)  # layout does not depend on batch / image size
        self._n_stages = lib.osi_resnet50_num_stages(probe.h)
        nparam = lib.osi_resnet50_param_floats(probe.h)
        nbuf = lib.osi_resnet50_buffer_floats(probe.h)
        nbn = lib.osi_resnet50_num_bn(probe.h)
        object.__setattr__(self, "_flat_params", torch.zeros(nparam))
        object.__setattr__(self, "_flat_grads", torch.zeros(nparam))
        object.__setattr__(self, "_flat_buffers", torch.zeros(nbuf))
        object.__setattr__(self, "_nbt", torch.zeros(nbn, dtype=torch.int64))
        object.__setattr__(self, "_anchor", torch.zeros(1, requires_grad=True))
        self._n_units = lib.osi_resnet50_num_units(probe.h)
        self._tunit = [lib.osi_resnet50_tensor_unit(probe.h, i) for i in range(lib.osi_resnet50_num_tensors(probe.h))]
        self._stage_ranges = []
        lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
        for s in range(self._n_stages):
            N.check(lib.osi_resnet50_stage_grad_range(probe.h, s, ctypes.byref(lo), ctypes.byref(hi)))
            self._stage_ranges.append((lo.value, hi.value))

        # ---- build the module tree + parameter views -------------------------------------------------------
        self._pinfo = []   # (name, offset, numel, shape)
        self._binfo = []   # (node, buffer name, arena name, offset, numel)
        name = ctypes.create_string_buffer(160)
        nd, shp, off, ne = ctypes.c_int(), (ctypes.c_int * 4)(), ctypes.c_size_t(), ctypes.c_size_t()
        bn_prefix = {}
        C, rm, rv = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        for j in range(nbn):
            N.check(lib.osi_resnet50_bn_info(probe.h, j, name, 160, ctypes.byref(C), ctypes.byref(rm), ctypes.byref(rv)))
            bn_prefix[name.value.decode()] = (j, C.value, rm.value, rv.value)
        for i in range(lib.osi_resnet50_num_tensors(probe.h)):
            N.check(lib.osi_resnet50_tensor_info(probe.h, i, name, 160, ctypes.byref(nd), shp, ctypes.byref(off), ctypes.byref(ne)))
            full = name.value.decode()
            shape = tuple(shp[k] for k in range(nd.value))
            self._pinfo.append((full, off.value, ne.value, shape))
            *path, leaf = full.split(".")
            node = self._node(path)
            node.register_parameter(leaf, nn.Parameter(self._view(self._flat_params, off.value, ne.value, shape)))
            prefix = ".".join(path)
            if leaf == "bias" and prefix in bn_prefix:
                j, c, rmo, rvo = bn_prefix[prefix]
                node.register_buffer("running_mean", self._flat_buffers[rmo:rmo + c])
                node.register_buffer("running_var", self._flat_buffers[rvo:rvo + c])
                node.register_buffer("num_batches_tracked", self._nbt[j])
                self._binfo += [(node, "running_mean", "_flat_buffers", rmo, c), (node, "running_var", "_flat_buffers", rvo, c),
                                (node, "num_batches_tracked", "_nbt", j, 0)]
        self.logits.in_features, self.logits.out_features = self._F, self._O
        self.resnet_base.fc.in_features, self.resnet_base.fc.out_features = 2048, self._F
        self._plist = [dict(self.named_parameters())[n] for (n, _, _, _) in self._pinfo]
        self._unit_names = {}      # unit -> "layerN.K" (bottlenecks), "fc" for the head
        for (full, _, _, _), u in zip(self._pinfo, self._tunit):
            parts = full.split(".")
            if 0 < u < self._n_units - 1 and u not in self._unit_names:
                self._unit_names[u] = parts[1] + "." + parts[2]
        self._unit_names[self._n_units - 1] = "fc"
        self._cut = 0              # freeze_below(): first trainable unit; 0 = nothing declared
        self._cut_froze = set()    # indices of the parameters whose requires_grad freeze_below() itself turned off
        self._plan_cache = {}      # requires_grad flag tuple -> (unit mask, stages that hold a trainable tensor)
        self._prefix_fwd = False   # the latest differentiable forward ran its frozen prefix in the inference form
        for p in self._plist:
            p._osi_owner = weakref.ref(self)
        self._nets = {}
        self._ws = None
        self._grad_sync = None   # set by dp.DistributedDataParallel
        self._fwd_serial = 0     # number of forward passes run; a backward must belong to the latest one
        self._grads_fresh = False  # a backward has filled the gradient arena since the last optimizer.zero_grad()
        self._bw_request = None    # next_backward(): (epsilon or None, lo, hi, accumulate, alpha or None, anchor, input_only) for the one
                                   # backward that follows; alpha is None for an FGSM request
        self._fw_request = None    # next_forward(): (partner, weight) of the mix the next differentiable forward applies at the cut
        self._adv_valid = False    # the latest backward wrote adversarial_batch()
        self._adv = {}             # (B, H, W) -> the model-owned PAIR of NHWC4 buffers the attack epilogues write: a backward writes the
                                   # one its forward did not read, so an attack can feed adversarial_batch() back without a copy
        self._adv_idx = {}         # (B, H, W) -> which of the pair was written last
        self._flat_grads2 = None   # second gradient arena of an accumulating backward
        self._bn_frozen = False    # freeze_bn(): BatchNorm on the running statistics (read-only) while the model is differentiated
        self._eval_plain = False   # the latest forward was an eval-mode inference forward run with grad enabled (no graph)
        self._fwd_input_only = False   # the latest forward ran under a pending next_backward(input_only=True)
        self._fwd_prefix = 0       # units the differentiable forward being set up runs in the inference forms (forward())
        self._bn_momentum = 0.1    # bn_momentum: handed to every executor that is not at the default (osi_resnet50_set_bn_momentum)
        self.reset_parameters()

    # ------------------------------------------------------------------------------------------------------
    def _node(self, path):
        node = self
        for comp in path:
            if comp not in node._modules:
                node.add_module(comp, _Node())
            node = node._modules[comp]
        return node

    @staticmethod
    def _view(arena, off, numel, shape):
        flat = arena[off:off + numel]
        if len(shape) == 4:  # logical OIHW over physical [O][H][W][I]
            o, i, h, w = shape
            return flat.view(o, h, w, i).permute(0, 3, 1, 2)
        return flat.view(shape)

    def reset_parameters(self):
        """torchvision's initialisation: kaiming-normal(fan_out, relu) convs, BN weight 1 / bias 0, default nn.Linear."""
        with torch.no_grad():
            for (name, _, _, shape), p in zip(self._pinfo, self._plist):
                if len(shape) == 4:
                    nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")
                elif len(shape) == 2:
                    nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                elif name.endswith("fc.bias") or name == "logits.bias":
                    fan_in = 2048 if name.endswith("fc.bias") else self._F
                    bound = 1 / math.sqrt(fan_in)
                    nn.init.uniform_(p, -bound, bound)
                elif name.endswith(".weight"):
                    p.fill_(1.0)
                else:
                    p.zero_()
            for node, bname, _, _, _ in self._binfo:
                buf = node._buffers[bname]
                buf.fill_(1.0) if bname == "running_var" else buf.zero_()

    # ---- device / dtype movement keeps the arenas whole ---------------------------------------------------
    def _apply(self, fn, recurse=True):
        new = {}
        for arena in ("_flat_params", "_flat_grads", "_flat_buffers"):
            t = fn(getattr(self, arena))
            if t.dtype != torch.float32:
                raise RuntimeError("the MI355X ResNet50 is fp32 only (parity dtype of the reference path)")
            new[arena] = t.contiguous()
        new["_nbt"] = fn(self._nbt).to(torch.int64)
        anchor = fn(self._anchor.detach()).requires_grad_(True)
        for k, v in new.items():
            object.__setattr__(self, k, v)
        object.__setattr__(self, "_anchor", anchor)
        with torch.no_grad():
            for (name, off, numel, shape), p in zip(self._pinfo, self._plist):
                had_grad = p.grad is not None
                p.data = self._view(self._flat_params, off, numel, shape)
                if had_grad:
                    p.grad = self._view(self._flat_grads, off, numel, shape)
            for node, bname, arena, off, c in self._binfo:
                src = getattr(self, arena)
                node._buffers[bname] = src[off] if arena == "_nbt" else src[off:off + c]
        self._ws = None
        self._adv, self._adv_idx, self._flat_grads2 = {}, {}, None
        return self

    # ---- arena access for the optimizer / DP layers -------------------------------------------------------
    def flat_parameters(self):
        return self._flat_params

    def flat_gradients(self):
        return self._flat_grads

    def gradient_buckets(self):
        """[(lo, hi)] float ranges of the gradient arena in the order backward finishes them (head first)."""
        return list(self._stage_ranges)

    def bind_gradients(self):
        """Point every parameter's .grad at its slice of the gradient arena; a parameter that does not require grad keeps
        .grad = None, as under autograd (the optimizers skip it)."""
        for (name, off, numel, shape), p in zip(self._pinfo, self._plist):
            if not p.requires_grad:
                p.grad = None
            elif p.grad is None or p.grad.data_ptr() != self._flat_grads.data_ptr() + 4 * off:
                p.grad = self._view(self._flat_grads, off, numel, shape)

    # ---- execution -------------------------------------------------------------------------------------------
    def _net(self, B, H, W):
        key = (B, H, W)
        if key not in self._nets:
            self._nets[key] = _Net(B, H, W, self._F, self._O, self._logit_bias)
            if self._bn_momentum != 0.1:
                N.ops().resnet50_set_bn_momentum(self._nets[key].h.value, self._bn_momentum)
        net = self._nets[key]
        dev = self._flat_params.device
        if self._ws is None or self._ws.numel() < net.ws_bytes or self._ws.device != dev:
            self._ws = None
            self._ws = torch.empty(net.ws_bytes, dtype=torch.uint8, device=dev)
        return net

    def _unit_of(self, first_trainable):
        """Unit index of a freeze_below() name: "layerN" (= its block 0), "layerN.K", "fc"."""
        by_name = {v: k for k, v in self._unit_names.items()}
        name = first_trainable
        if isinstance(name, str) and name + ".0" in by_name:
            name = name + ".0"
        if not isinstance(name, str) or name not in by_name:
            raise ValueError(f"freeze_below: {first_trainable!r} is not a cut; expected 'layer1' .. 'layer4', 'layerN.K' with an "
                             "existing block K, 'fc', or None")
        return by_name[name]

    def freeze_below(self, first_trainable):
        """Declare that everything before `first_trainable` is frozen ENTIRELY — weights, BatchNorm affine parameters and BatchNorm
        statistics — which is what `.eval()` plus `requires_grad_(False)` on those sub-modules means in torch; returns self.
        `first_trainable`: "layer1" .. "layer4" (that layer's block 0 is the first trainable unit), "layerN.K" (that block), "fc" (head
        only), None (clears the declaration). The prefix's parameters get requires_grad_(False); parameters an earlier call froze and
        that are no longer in the prefix get requires_grad_(True) back; no other flag is touched. While a cut is declared a
        differentiable forward runs the prefix in the inference forms on the running statistics (no backward state, no statistics
        update); the suffix follows the model's mode: batch statistics in train(), running statistics under freeze_bn() or eval."""
        cut = 0 if first_trainable is None else self._unit_of(first_trainable)
        for i, (p, u) in enumerate(zip(self._plist, self._tunit)):
            if u < cut:
                if p.requires_grad:
                    p.requires_grad_(False)
                    self._cut_froze.add(i)
            elif i in self._cut_froze:
                p.requires_grad_(True)
                self._cut_froze.discard(i)
        self._cut = cut
        return self

    @property
    def frozen_below(self):
        """Canonical name of the declared cut ("layerN.K" or "fc"), None when nothing is declared (read-only)."""
        return self._unit_names[self._cut] if self._cut else None

    def _trainable_plan(self):
        """(unit mask, per backward stage: does its gradient range hold a trainable tensor) from the requires_grad flags, cached on
        the flag tuple. The units come from the executor's table (osi_resnet50_tensor_unit), not from the names."""
        flags = tuple(p.requires_grad for p in self._plist)
        plan = self._plan_cache.get(flags)
        if plan is None:
            mask = 0
            live = [False] * self._n_stages
            for f, u, (_, off, _, _) in zip(flags, self._tunit, self._pinfo):
                if f:
                    mask |= 1 << u
                    for s, (lo, hi) in enumerate(self._stage_ranges):
                        if lo <= off < hi:
                            live[s] = True
            if len(self._plan_cache) > 64:
                self._plan_cache.clear()
            plan = self._plan_cache[flags] = (mask, tuple(live))
        return plan

    def _set_trainable(self, net, mask, prefix):
        """Hand (unit mask, inference-form prefix) to the executor of this geometry when it changed."""
        full = (1 << self._n_units) - 1
        want = (mask or full, prefix)        # no trainable parameter at all: the backward runs input-only, the mask plays no part
        if (net.trainable or (full, 0)) == want:
            return
        if net.owes_backward:   # a differentiable forward that never got its backward: give its state up, the setting may change then
            N.check(N.lib().osi_resnet50_set_option(net.h, b"forget_forward", 1), "osi_resnet50_set_option(forget_forward)")
            net.owes_backward = False
        N.check(N.lib().osi_resnet50_set_trainable(net.h, want[0], want[1]), "osi_resnet50_set_trainable")
        net.trainable = want

    def freeze_bn(self, mode=True):
        """Freeze (mode=True) or release the BatchNorm statistics of the WHOLE model; returns self. Frozen: every differentiable forward
        normalises with the running statistics and neither updates them nor num_batches_tracked (fine-tuning on small batches keeps the
        checkpoint's statistics), and its backward is the frozen form dy = gamma * invstd * g. `model.training` keeps its meaning;
        in eval mode the statistics are frozen anyway (see forward)."""
        self._bn_frozen = bool(mode)
        return self

    @property
    def bn_frozen(self):
        """True after freeze_bn() (read-only; eval mode differentiates on the running statistics without it)."""
        return self._bn_frozen

    @property
    def bn_momentum(self):
        """The running-statistics update factor of every BatchNorm in a training-mode forward: running = (1 - m) * running + m * batch,
        m in (0, 1], default 0.1 (torch's). Applied to every executor the model has created and will create; it takes effect at the
        next training-mode forward. Frozen and inference forwards never read it. 1.0 leaves the batch statistics in the buffers; 1 / k
        before batch k is the cumulative average of averaging.update_bn."""
        return self._bn_momentum

    @bn_momentum.setter
    def bn_momentum(self, value):
        value = float(value)
        if not 0.0 < value <= 1.0:        # a NaN fails both comparisons
            raise ValueError(f"bn_momentum must lie in (0, 1], got {value!r}")
        for net in self._nets.values():
            N.ops().resnet50_set_bn_momentum(net.h.value, value)
        self._bn_momentum = value

    def next_backward(self, fgsm=None, lo=0.0, hi=1.0, accumulate=False, *, pgd=None, input_only=False):
        """Request for the ONE backward that follows (whatever route it takes: a fused loss's plain backward(), autograd):
          fgsm = epsilon   its last stage also writes the adversarial batch clamp(x + epsilon * sign(dJ/dx), lo, hi) from the input the
                           forward read (NCHW, NHWC4 or uint8-staged alike) into a model-owned NHWC4 buffer: adversarial_batch();
                           dJ/dimage itself is never written (osi_resnet50_backward_adv);
          pgd = (alpha, epsilon, anchor)   one step of a projected attack instead (osi_resnet50_backward_attack): the input the forward
                           read is the iterate x, adversarial_batch() receives
                           clamp(min(max(x + alpha * sign(dJ/dx), a - epsilon), a + epsilon), lo, hi) with a = `anchor`, the clean batch
                           as NHWC4 fp32 [B, H, W, 4] of the forward's geometry on the model's device (adversary.as_nhwc4), or None: the
                           forward's own input (step 0). alpha is finite (negative descends), epsilon >= 0 (inf: no projection).
                           Mutually exclusive with fgsm;
          input_only       (with fgsm or pgd, not with accumulate) the backward computes NO parameter gradient: the gradient arena,
                           every p.grad and the optimizers' "fresh gradients" mark stay as they are, nothing runs on the weight-gradient
                           side stream, and under data parallel no bucket is handed to the gradient sync and no collective runs. The
                           inner steps of a multi-step attack and attacks inside validate(). This request has to PRECEDE its forward in
                           every mode: a backward that finds the request but whose forward ran without it raises RuntimeError;
          accumulate       its parameter gradients go into a second arena that is then added into the first (osi_grad_accumulate), so
                           p.grad holds the sum of this backward and the one before it, as autograd's accumulation would leave it.
        The adversarial buffer is a pair per geometry: a backward writes the one its forward did not read, adversarial_batch() is the
        one written last, so feeding adversarial_batch() back k times needs no copy (the batch of two steps ago is overwritten).
        In eval mode (without freeze_bn()) the request has to PRECEDE the forward: it is what makes that forward differentiable (a plain
        eval-mode forward builds no graph). A request that arrives after such a forward raises; run plain eval-mode forwards under
        torch.no_grad(), as validate() does, when requests for later forwards follow them."""
        if fgsm is not None and pgd is not None:
            raise ValueError("next_backward: fgsm and pgd are mutually exclusive")
        alpha = anchor = None
        if pgd is not None:
            alpha, fgsm, anchor = pgd
            alpha = float(alpha)
            if not math.isfinite(alpha):
                raise ValueError("next_backward: pgd alpha must be finite")
            if anchor is not None:
                if not isinstance(anchor, torch.Tensor) or not self._is_nhwc4(anchor) or anchor.device != self._flat_params.device:
                    raise ValueError("next_backward: the pgd anchor must be None or an NHWC4 fp32 batch [B, H, W, 4] on the model's device "
                                     "(adversary.as_nhwc4)")
                anchor = anchor.detach().contiguous()
        if input_only:
            if fgsm is None or accumulate:
                raise ValueError("next_backward(input_only=True) goes with fgsm or pgd and not with accumulate: an input-only backward "
                                 "produces the adversarial batch and nothing else")
        if fgsm is not None and self._prefix_fwd and getattr(self, "_last", None) is not None and self._last[0].owes_backward:
            raise RuntimeError("next_backward(fgsm=...): the latest forward ran the prefix frozen by freeze_below() in the inference form, which "
                               "keeps nothing to differentiate; call next_backward(fgsm=...) BEFORE the forward it belongs to")
        if (fgsm is not None or accumulate) and not input_only and self._eval_plain and not self.training and not self._bn_frozen:
            raise RuntimeError("next_backward(): the latest forward was an eval-mode inference forward, which keeps nothing to differentiate; "
                               "in eval mode call next_backward(...) BEFORE the forward it belongs to (or freeze_bn() / requires_grad_ on "
                               "the image), and run plain eval-mode forwards under torch.no_grad()")
        if fgsm is not None and not float(fgsm) >= 0.0:
            raise ValueError("next_backward: epsilon must be >= 0")
        if not float(lo) <= float(hi):
            raise ValueError("next_backward: lo <= hi")
        self._bw_request = (None if fgsm is None else float(fgsm), float(lo), float(hi), bool(accumulate), alpha, anchor, bool(input_only))

    def next_forward(self, mix=None):
        """Request for the ONE differentiable forward that follows (beside next_backward):
          mix = (partner, weight)   manifold mixup at the cut declared with freeze_below(): after the frozen prefix has written the input
                           of the first trainable block and before that block reads it, the rows of that tensor are mixed pairwise in
                           place (osi_mix_rows_pairs): row i becomes weight[i] * x_i + (1 - weight[i]) * x_partner[i], a row that is its own
                           partner stays as it is. partner: int32, weight: fp32, device tensors of B entries (the batch of that forward);
                           partner is an involution (partner[partner[i]] == i). The suffix trains on the mixed activations; the prefix is
                           frozen, so no gradient crosses the mix. None clears a pending request.
        Raises ValueError when no block cut is declared (frozen_below is None or "fc"). The forward raises RuntimeError when it would not
        run the prefix in the inference form — an image that requires grad, a pending attack request, no trainable parameter — and the
        request stays pending (next_forward(mix=None) clears it). A no-grad or inference forward ignores the request and leaves it pending."""
        if mix is None:
            self._fw_request = None
            return
        if not 0 < self._cut < self._n_units - 1:
            raise ValueError(f"next_forward(mix=...): the mix lives at the input of the first trainable block, but frozen_below is "
                             f"{self.frozen_below!r}; declare a block cut with freeze_below('layer1' .. 'layer4' or 'layerN.K') first")
        try:
            partner, weight = mix
        except (TypeError, ValueError):
            raise TypeError("next_forward: mix must be a pair (partner, weight) of device tensors") from None
        if not isinstance(partner, torch.Tensor) or not isinstance(weight, torch.Tensor):
            raise TypeError("next_forward: mix must be a pair (partner, weight) of device tensors")
        if partner.dtype != torch.int32 or weight.dtype != torch.float32:
            raise TypeError(f"next_forward: mix partner must be int32 and weight float32, got {partner.dtype} and {weight.dtype}")
        if partner.dim() != 1 or weight.dim() != 1 or partner.shape != weight.shape:
            raise ValueError(f"next_forward: mix partner and weight must be vectors of one length (the batch), got shapes "
                             f"{tuple(partner.shape)} and {tuple(weight.shape)}")
        dev = self._flat_params.device
        if not partner.is_cuda or partner.device != dev or weight.device != dev:
            raise ValueError("next_forward: mix partner and weight must live on the model's device (the MI355X build has no CPU path)")
        self._fw_request = (partner.detach().contiguous(), weight.detach().contiguous())

    def adversarial_batch(self):
        """The NHWC4 batch [B, H, W, 4] written by the latest backward that ran under next_backward(fgsm=... / pgd=...). Model-owned:
        one of a pair per geometry, overwritten by the second such backward after this one; feed it to the model as it is."""
        last = getattr(self, "_last", None)
        shape = net_shape(self, last[0]) if last is not None else None
        pair = self._adv.get(shape)
        if pair is None or not self._adv_valid:
            raise RuntimeError("adversarial_batch(): the latest backward did not run under next_backward(fgsm=... / pgd=...)")
        return pair[self._adv_idx[shape]]

    def pooled(self):
        """The penultimate activation of this module's latest forward: the [B, 2048] average-pooled output of layer4 (non-negative),
        a new device tensor copied out of the executor's workspace (osi_resnet50_pooled). features = fc(pooled), bit for bit. Valid
        after a forward of any kind (train, eval, frozen) until the next one; ValueError before any forward."""
        last = getattr(self, "_last", None)
        if last is None or self._ws is None:
            raise ValueError("pooled(): this module has not run a forward yet")
        return N.ops().resnet50_pooled(last[0].h.value, self._ws)

    def mark_gradients_ready(self):
        """Tell the fused optimizers that the gradient arena was filled by hand (tests, custom loops) rather than by backward()."""
        self._grads_fresh = True

    @staticmethod
    def _is_nhwc4(image):
        """fp32 [B, H, W, 4] batch already in the executor's input layout (written by pipeline.DevicePrefetcher)."""
        return image.dtype == torch.float32 and image.dim() == 4 and image.shape[3] == 4 and image.shape[1] != 3

    def _check_image(self, image):
        if isinstance(image, torch.Tensor) and image.dtype == torch.uint8:   # decoded RGB batch, staged on the device
            if image.dim() != 4 or image.shape[3] != 3:
                raise ValueError("a uint8 image batch must be [B, H, W, 3] (decoded RGB rows)")
        elif isinstance(image, torch.Tensor) and self._is_nhwc4(image):
            pass
        elif not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[1] != 3:
            raise ValueError("expected an image batch [B, 3, H, W]")
        if not image.is_cuda or not self._flat_params.is_cuda:
            raise RuntimeError("openset_imagenet (MI355X build) has no CPU path: move the model and the batch to the GPU "
                               "(set_device_gpu(index); device(model); device(images)).")
        if image.device != self._flat_params.device:
            raise RuntimeError("image batch and model live on different devices")
        if image.dtype not in (torch.float32, torch.uint8):
            raise TypeError("image batch must be float32 [B,3,H,W] (reference: ToTensor(), train.py:259-263) or uint8 [B,H,W,3]")

    def _run_forward(self, image, want_grad, flip=None, frozen=False):
        image = image.contiguous()
        staged = image.dtype == torch.uint8
        bound = not staged and self._is_nhwc4(image)
        if staged or bound:
            B, H, W, _ = image.shape
        else:
            B, _, H, W = image.shape
        net = self._net(B, H, W)
        if want_grad:    # the executor learns which units are trainable, and how much of the frozen prefix runs the inference forms
            self._set_trainable(net, self._trainable_plan()[0], self._fwd_prefix)
        mix = self._fw_request if want_grad else None
        if mix is not None and mix[0].numel() != B:
            raise ValueError(f"next_forward: mix partner and weight hold {mix[0].numel()} entries, the batch has {B} rows")
        if staged and flip is not None:   # ToTensor + horizontal flip + NHWC4 staging in one pass on the device (osi_u8hwc3_to_nhwc4)
            flip = torch.as_tensor(flip).to(device=image.device, dtype=torch.uint8).contiguous()
            if flip.numel() != B:
                raise ValueError("flip must hold one flag per image")
        elif flip is not None:
            raise ValueError("flip flags are only meaningful with a uint8 [B,H,W,3] batch")
        # one custom op = the whole network on the current HIP stream: uint8 batches are staged, NHWC4 batches bound in place
        # (conv1 forward now, conv1 weight gradient at the end of this step's backward), NCHW batches converted on the way in
        if mix is not None:   # one-shot: the executor mixes the input of the first trainable block in this forward (osi_resnet50_set_mix)
            N.ops().resnet50_set_mix(net.h.value, mix[0], mix[1])
            self._fw_request = None
        try:
            if frozen:   # the training topology on the running statistics (read-only), differentiable: osi_resnet50_forward_frozen
                logits, features = N.ops().resnet50_forward_frozen(net.h.value, self._flat_params, self._flat_buffers, image, flip, self._ws,
                                                                   self._F, self._O)
            else:
                logits, features = N.ops().resnet50_forward(net.h.value, self._flat_params, self._flat_buffers, self._nbt, image, flip,
                                                            self._ws, self._F, self._O, bool(self.training and not self._bn_frozen))
        except Exception:
            if mix is not None:   # a forward that failed before it ran leaves the executor's request pending: take it back
                N.ops().resnet50_set_mix(net.h.value, None, None)
            raise
        self._eval_plain = not frozen and not self.training and torch.is_grad_enabled()
        self._fwd_input_only = bool(want_grad) and self._bw_request is not None and self._bw_request[6]
        # (any forward replaces the executor's backward state; only a differentiable one leaves a backward owed)
        net.owes_backward = bool(want_grad)
        self._prefix_fwd = bool(want_grad) and self._fwd_prefix > 0
        self._fwd_serial += 1
        self._last = (net, image if (want_grad or bound) else None)   # keeps a bound batch alive until the next forward
        return logits, features

    def _run_backward(self, dlogits, dfeatures, want_image=False, param_grads=True):
        """Backward of the latest forward. want_image: also return dJ/dimage (NCHW fp32, the forward's batch geometry);
        param_grads = False: input-only backward (no parameter gradient is computed, the gradient arena is not touched)."""
        net, fwd_image = self._last
        B, H, W = net_shape(self, net)
        if dlogits is None:
            dlogits = torch.zeros(B, self._O, device=self._flat_params.device)
        dlogits = dlogits.contiguous().float()
        dfeatures = None if dfeatures is None else dfeatures.contiguous().float()
        dimage = torch.empty(B, 3, H, W, device=self._flat_params.device) if want_image else None
        sync = self._grad_sync
        request, self._bw_request = self._bw_request, None
        eps, clamp_lo, clamp_hi, accumulate, alpha, anchor, input_only = request if request is not None else (None, 0.0, 1.0, False, None, None, False)
        self._adv_valid = False
        if input_only:    # the request decides: no parameter gradient, whatever the graph says about the parameters
            if not self._fwd_input_only:
                raise RuntimeError("next_backward(input_only=True) has to PRECEDE the forward it belongs to: the latest forward was set "
                                   "up for a backward with parameter gradients")
            if want_image:
                raise ValueError("next_backward(input_only=True) builds the adversarial batch inside the backward: the image batch must "
                                 "not require grad as well (dJ/dimage is not written on that path)")
            param_grads = False
        if (eps is not None or accumulate) and not param_grads and not input_only:
            raise RuntimeError("next_backward(): the requested backward computes parameter gradients, but every parameter is frozen")
        if eps is not None and want_image:
            raise ValueError("next_backward(fgsm=...) builds the adversarial batch inside the backward: the image batch must not require "
                             "grad as well (dJ/dimage is not written on that path)")
        if accumulate and not self._grads_fresh:
            raise RuntimeError("next_backward(accumulate=True): no backward has filled the gradient arena since zero_grad()")
        dev = self._flat_params.device
        if accumulate and (self._flat_grads2 is None or self._flat_grads2.device != dev):
            self._flat_grads2 = torch.zeros_like(self._flat_grads)   # zeros: the alignment gaps between tensors are never written
        if eps is not None:
            pair = self._adv.get((B, H, W))
            if pair is None or pair[0].device != dev:
                pair = self._adv[(B, H, W)] = (torch.empty(B, H, W, 4, device=dev), torch.empty(B, H, W, 4, device=dev))
            # the buffer the forward did not read (a forward on anything else: the first)
            out = 1 if fwd_image is not None and fwd_image.data_ptr() == pair[0].data_ptr() else 0
            x_adv = pair[out]
            assert fwd_image is None or fwd_image.data_ptr() != x_adv.data_ptr(), "the attack epilogue would overwrite its forward's input"
            if alpha is None and not input_only:
                adv = N.ops().resnet50_backward_adv
                bwd = lambda *a: adv(*a[:6], x_adv, eps, clamp_lo, clamp_hi, *a[6:])
            else:         # ABI 19: the projected step and / or the input-only form (an FGSM step is alpha = epsilon around the iterate)
                attack = N.ops().resnet50_backward_attack
                step = eps if alpha is None else alpha
                bwd = lambda *a: attack(*a[:6], x_adv, anchor, step, eps, clamp_lo, clamp_hi, bool(param_grads), *a[6:])
        elif dimage is None and param_grads:
            bwd = N.ops().resnet50_backward
        else:             # ABI 8: dJ/dimage written by the last stage, and/or no parameter gradient
            ex = N.ops().resnet50_backward_ex
            bwd = lambda *a: ex(*a[:6], dimage, bool(param_grads), *a[6:])
        grads = self._flat_grads if param_grads else self._flat_grads[:0]
        if accumulate:    # into the second arena (under data parallel its buckets are averaged on their own), added into the first below
            grads = self._flat_grads2
        if sync is None or input_only:  # single GPU: all stages in one call (one side-stream join at the end); an input-only attack step
                                        # under data parallel as well: there is no gradient to average, the sync never hears of it
            bwd(net.h.value, self._flat_params, grads, self._ws, dlogits, dfeatures, 0, self._n_stages)
        else:             # data parallel: stage by stage, each finished slice of the gradient arena goes to the all-reduce
            if not net.staged:   # staged calls no longer join the weight-gradient side stream into the compute stream (only the last does)
                N.check(N.lib().osi_resnet50_set_option(net.h, b"stage_join", 0), "osi_resnet50_set_option(stage_join)")
                net.staged = True
            handoff = lambda comm: N.ops().resnet50_grads_ready(net.h.value, grads, comm.cuda_stream)
            live = self._trainable_plan()[1]
            for s in range(self._n_stages):
                bwd(net.h.value, self._flat_params, grads, self._ws, dlogits, dfeatures, s, s + 1)
                # input-only: no parameter gradient to average; a stage without a trainable tensor: nobody reads its slice
                if param_grads and live[s]:
                    lo, hi = self._stage_ranges[s]
                    sync.bucket_ready(grads, lo, hi, handoff)
            sync.finish()
        net.owes_backward = False
        if accumulate:
            N.ops().grad_accumulate(self._flat_grads, grads)
        self._adv_valid = eps is not None
        if eps is not None:
            self._adv_idx[(B, H, W)] = out
        if param_grads:
            self._grads_fresh = True
            self.bind_gradients()
        return dimage

    def forward(self, image, flip=None):
        """Forward pass: returns (logits, deep features) like the reference (model.py:28-39).

        `image` is the reference's fp32 [B,3,H,W] batch in [0,1], or — the device-side input pipeline — a uint8 [B,H,W,3] batch
        of decoded, cropped RGB rows with optional per-image horizontal-flip flags (ToTensor(), RandomHorizontalFlip and the
        layout staging then happen in one pass on the GPU and the host link carries a quarter of the bytes), or an fp32
        [B,H,W,4] batch already staged in the executor's layout by pipeline.DevicePrefetcher (read in place).

        With grad enabled: in training mode the forward is differentiable on batch statistics (which it updates) — unless freeze_bn()
        is on: then, and in eval mode whenever something asks for a gradient (freeze_bn(), an image that requires grad, a pending
        next_backward(...) request), it is differentiable on the running statistics, which it leaves untouched (the frozen route).
        Every other eval-mode forward is the inference forward without a graph. Under a pending next_backward(input_only=True) the graph
        exists for the attack alone: its backward computes no parameter gradient, whatever the parameters' requires_grad flags say."""
        self._check_image(image)
        frozen = self._bn_frozen or not self.training
        differentiable = self.training or self._bn_frozen or image.requires_grad or self._bw_request is not None
        if torch.is_grad_enabled() and differentiable:
            image_grad = image.requires_grad
            if image_grad and self._is_nhwc4(image):
                raise ValueError("only NCHW fp32 [B, 3, H, W] image batches are differentiable; an NHWC4 batch "
                                 "(pipeline.DevicePrefetcher's layout) cannot require grad")
            param_grad = self._plist[0].requires_grad or any(p.requires_grad for p in self._plist)
            self._fwd_prefix = 0
            if self._cut and (param_grad or image_grad):
                for p, u, (name, _, _, _) in zip(self._plist, self._tunit, self._pinfo):
                    if u < self._cut and p.requires_grad:
                        raise RuntimeError(f"freeze_below({self.frozen_below!r}) is declared, but parameter {name} of the frozen prefix "
                                           "requires grad; clear the declaration with freeze_below(None) or move the cut")
                if image_grad or (self._bw_request is not None and self._bw_request[0] is not None):
                    if not frozen:
                        raise RuntimeError("image gradients through a prefix frozen by freeze_below() need freeze_bn() or eval mode: under a "
                                           "batch-statistics suffix the prefix keeps no backward state")
                    # frozen route: the full frozen topology, the backward runs to full depth (frozen units get no weight gradient)
                else:
                    self._fwd_prefix = self._cut
            input_only = self._bw_request is not None and self._bw_request[6]
            if self._fw_request is not None and not 0 < self._fwd_prefix < self._n_units - 1:
                raise RuntimeError("next_forward(mix=...) is pending, but this forward does not run a frozen prefix below a block cut (an image "
                                   "that requires grad, a pending attack request, no trainable parameter, or the cut was moved): the mix has "
                                   "no place in it; next_forward(mix=None) clears the request")
            if param_grad or image_grad or input_only:
                # no parameter requires grad: a detached anchor, so the backward runs input-only. A pending input-only attack request
                # needs a graph even then (the anchor is a stand-in leaf: no parameter is part of the graph either way)
                anchor = self._anchor if (param_grad or input_only) else self._anchor.detach()
                return _BackboneFn.apply(image, anchor, self, flip, frozen)
        return self._run_forward(image, False, flip)


def freeze_below_of(cfg):
    """The optional top-level config key `freeze_below` (a cut name of ResNet50.freeze_below; absent, null or off = none): the name, or
    None. The name itself is checked by ResNet50.freeze_below when it is applied."""
    value = getattr(cfg, "freeze_below", None)
    if value is None or value is False or (isinstance(value, str) and value.lower() in ("", "off", "none", "null", "false", "no")):
        return None
    if not isinstance(value, str):
        raise ValueError(f"freeze_below: expected a cut name ('layer1' .. 'layer4', 'layerN.K', 'fc'), got {value!r}")
    return value


def net_shape(model, net):
    for (B, H, W), n in model._nets.items():
        if n is net:
            return B, H, W
    raise RuntimeError("unknown executor")

"""An averaged copy of the weights beside the model that trains: EMA (the exponential moving average torchvision / timm recipes
evaluate and ship) and SWA (the equal-weight average of the late epochs, followed by a BatchNorm re-estimation pass).

  AveragedModel(model, kind="ema" | "swa", decay=0.999, buffers="copy" | "average")     torch.optim.swa_utils.AveragedModel
      .module                      a second, complete model: validate(), get_arrays(), load_state_dict, attacks all take it
      .update_parameters(model)    avg = lerp(avg, model, weight): ONE osi_average_update launch over the arenas of a ResNet50
      .state_dict() / .load_state_dict()    torch's schema: `n_averaged`, `module.<reference key>`
  update_bn(loader, model)         torch.optim.swa_utils.update_bn for a ResNet50 (or an AveragedModel of one): the cumulative average of
                                   the batch statistics through the executor's BatchNorm momentum (ResNet50.bn_momentum = 1 / k)
  options(cfg) / build(cfg, model) the optional config block `avg:` of the training loop (train.train, train.worker)

torch's own AveragedModel does not work on this package's ResNet50: its 162 tensors are views into one flat arena, which deepcopy
breaks, and a per-tensor foreach update would be 160+ small launches per step beside the hand-written path.
"""
import copy

import torch
from torch import nn

from . import _native as N
from . import dp as _dp
from .model import ResNet50

KINDS = ("ema", "swa")
BUFFERS = ("copy", "average")


def _unwrap(model):
    return model.module if isinstance(model, (_dp.DistributedDataParallel, torch.nn.parallel.DistributedDataParallel)) else model


class AveragedModel(nn.Module):
    """Averaged weights of `model` (a ResNet50 of this package, or any nn.Module).

    kind = "ema": avg = decay * avg + (1 - decay) * model per update; "swa": the equal-weight mean of the models seen at the updates
    (`decay` is not used). The first update_parameters() copies. The arithmetic is torch.lerp's on fp32, so the result is bit-equal
    to torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay) / get_swa_multi_avg_fn().

    `.module` of a ResNet50 is BUILT — ResNet50(fc_layer_dim, out_features, logit_bias) on the model's device, with arenas of its
    own — and then filled from the model's arenas; it is never a deepcopy (which would break the views into the arenas). One update
    is one osi_average_update launch over `_flat_params` (and `_flat_buffers` under buffers="average"); there is no CPU path for
    it. Any other nn.Module is deep-copied and updated with torch._foreach_lerp_ as swa_utils does.

    buffers = "copy" (torch's use_buffers=False): the buffers — BatchNorm running statistics — are the model's latest after every
    update. "average" (use_buffers=True): the floating-point buffers are averaged with the weight of the parameters.
    `num_batches_tracked` (every non-floating buffer) is always copied: torch's integer "average" of that counter under
    use_buffers=True is not reproduced.

    `n_averaged` is a host integer, mirrored in the registered buffer of that name (torch's), which lives on the host: an update
    neither synchronises nor allocates on the device. Under data parallel no collective is needed: every rank holds the same
    parameters after a step; buffers="copy" takes the rank's own statistics."""

    def __init__(self, model, kind="ema", decay=0.999, buffers="copy"):
        super().__init__()
        if kind not in KINDS:
            raise ValueError(f"AveragedModel: kind must be one of {KINDS}, got {kind!r}")
        if buffers not in BUFFERS:
            raise ValueError(f"AveragedModel: buffers must be one of {BUFFERS}, got {buffers!r}")
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"AveragedModel: decay must lie in [0, 1], got {decay!r}")
        self.kind, self.decay, self.buffers_mode = kind, decay, buffers
        model = _unwrap(model)
        if isinstance(model, ResNet50):
            self.module = ResNet50(model._F, model._O, model._logit_bias).to(model._flat_params.device)
            self.module.train(model.training)
        else:
            self.module = copy.deepcopy(model)
        self.register_buffer("n_averaged", torch.tensor(0, dtype=torch.long))
        self.restart(model)

    @torch.no_grad()
    def restart(self, model):
        """Start the average afresh from `model`: `.module` holds its parameters and buffers, n_averaged = 0 (what the constructor
        leaves; a deep copy already holds them)."""
        model = _unwrap(model)
        if isinstance(self.module, ResNet50):
            self.module._flat_params.copy_(model._flat_params)
            self.module._flat_buffers.copy_(model._flat_buffers)
            self.module._nbt.copy_(model._nbt)
        else:
            for a, m in zip(list(self.module.parameters()) + list(self.module.buffers()), list(model.parameters()) + list(model.buffers())):
                a.detach().copy_(m.detach())
        self._n = 0
        self.n_averaged.zero_()

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def _weight(self):
        """lerp weight of the next update: 1 copies; swa's 1 / (n + 1) is evaluated in double, as the Python float torch hands to lerp"""
        if self._n == 0:
            return 1.0
        return 1.0 - self.decay if self.kind == "ema" else 1.0 / (self._n + 1)

    @torch.no_grad()
    def update_parameters(self, model):
        model = _unwrap(model)
        weight = self._weight()
        avg = self.module
        if isinstance(avg, ResNet50):
            if not isinstance(model, ResNet50) or model._flat_params.numel() != avg._flat_params.numel():
                raise TypeError("AveragedModel.update_parameters: expected the ResNet50 this average was built from")
            if self.buffers_mode == "average":
                N.ops().average_update([avg._flat_params, avg._flat_buffers], [model._flat_params, model._flat_buffers], weight)
            else:
                N.ops().average_update([avg._flat_params], [model._flat_params], weight)
                avg._flat_buffers.copy_(model._flat_buffers)
            avg._nbt.copy_(model._nbt)
        else:
            pairs = list(zip(avg.parameters(), model.parameters()))
            copies = []
            for b_avg, b_model in zip(avg.buffers(), model.buffers()):
                if self.buffers_mode == "average" and b_avg.is_floating_point():
                    pairs.append((b_avg, b_model))
                else:
                    copies.append((b_avg, b_model))
            floating = [(a.detach(), m.detach().to(a.device)) for a, m in pairs if a.is_floating_point() or a.is_complex()]
            copies += [(a, m) for a, m in pairs if not (a.is_floating_point() or a.is_complex())]
            if self._n == 0:
                copies += floating
            elif floating:
                torch._foreach_lerp_([a for a, _ in floating], [m for _, m in floating], weight)
            for a, m in copies:
                a.detach().copy_(m.detach())
        self._n += 1
        self.n_averaged.fill_(self._n)

    def load_state_dict(self, state_dict, *args, **kwargs):
        out = super().load_state_dict(state_dict, *args, **kwargs)
        self._n = int(self.n_averaged)
        return out

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.n_averaged = self.n_averaged.cpu()      # the counter stays on the host: an update does not touch the device for it
        return self


@torch.no_grad()
def update_bn(loader, model):
    """torch.optim.swa_utils.update_bn for a ResNet50 or an AveragedModel of one: running_mean = 0, running_var = 1,
    num_batches_tracked = 0, then one training-mode forward per batch of `loader` (the batch forms train() accepts) with the executor's
    BatchNorm momentum set to 1 / k before batch k = 1, 2, ... — the cumulative average torch's momentum = None gives. The host counts:
    nothing is read back. The model's bn_momentum and training flag are restored afterwards, also when an exception occurs; the
    parameters are not touched. ValueError under freeze_bn() or a declared freeze_below(): part of the statistics would not move."""
    from .pipeline import device_batch
    net = _unwrap(model)
    if isinstance(net, AveragedModel):
        net = net.module
    if not isinstance(net, ResNet50):
        raise TypeError("update_bn: expected a ResNet50 of this package or an AveragedModel of one (torch.optim.swa_utils.update_bn "
                        "serves every other module)")
    if net.bn_frozen or net.frozen_below is not None:
        raise ValueError("update_bn: the model's BatchNorm statistics are frozen (freeze_bn() / freeze_below()); release them first")
    fresh = torch.zeros(net._flat_buffers.numel())
    for _, bname, arena, off, c in net._binfo:
        if arena == "_flat_buffers" and bname == "running_var":
            fresh[off:off + c] = 1.0
    net._flat_buffers.copy_(fresh)
    net._nbt.zero_()
    was_training, momentum = net.training, net.bn_momentum
    ran = False
    try:
        net.train()
        for k, batch in enumerate(loader, 1):
            net.bn_momentum = 1.0 / k
            images = batch if isinstance(batch, torch.Tensor) else device_batch(batch)[0]
            net(images.to(net._flat_params.device, non_blocking=True))
            ran = True
    finally:
        net.bn_momentum = momentum
        net.train(was_training)
        last = getattr(net, "_last", None)
        if ran and last is not None:      # the training-mode forwards above get no backward: the executor gives their state up
            N.check(N.lib().osi_resnet50_set_option(last[0].h, b"forget_forward", 1), "osi_resnet50_set_option(forget_forward)")


# ---- the optional config block `avg:` ----------------------------------------------------------------------------------------------
_KEYS = ("kind", "decay", "every", "start_epoch", "buffers", "select", "update_bn")


class Options:
    """The checked values of an `avg:` block (options())."""

    def __init__(self, kind, decay, every, start_epoch, buffers, select, update_bn):
        self.kind, self.decay, self.every, self.start_epoch = kind, decay, every, start_epoch
        self.buffers, self.select, self.update_bn = buffers, select, update_bn

    def __repr__(self):
        return "avg(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in _KEYS) + ")"


def _on_off(value, key):
    if isinstance(value, bool):
        return value
    if isinstance(value, str) and value.lower() in ("on", "off", "true", "false", "yes", "no"):
        return value.lower() in ("on", "true", "yes")
    raise ValueError(f"avg.{key}: expected on / off, got {value!r}")


def options(cfg):
    """The optional config block `avg:` as Options, None when it is absent or `kind: off` (then the run is the one without it).
        kind: ema | swa | off     decay: 0.9998 (ema, in [0, 1])     every: 1 (optimizer steps per update, integer >= 1)
        start_epoch: 0 (averaging begins with this epoch; swa: the late phase)     buffers: copy | average
        select: model | averaged (whose validation score drives _best.pth and early stopping)
        update_bn: off | on (after the last epoch: update_bn(train_loader, averaged), one more validation, {name}_avg.pth)
    ValueError on anything else, when the loop is set up."""
    block = getattr(cfg, "avg", None)
    if block is None:
        return None
    values = dict(block) if isinstance(block, dict) else dict(vars(block)) if hasattr(block, "__dict__") else None
    if values is None:
        raise ValueError(f"avg: expected a mapping, got {block!r}")
    unknown = sorted(set(values) - set(_KEYS))
    if unknown:
        raise ValueError(f"avg: unknown key(s) {unknown}; expected {list(_KEYS)}")
    kind = values.get("kind", "ema")
    if kind is False or (isinstance(kind, str) and kind.lower() == "off"):       # (YAML reads a bare `off` as False)
        kind = "off"
    if kind not in KINDS + ("off",):
        raise ValueError(f"avg.kind must be ema, swa or off, got {kind!r}")
    decay = values.get("decay", 0.9998)
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:
        raise ValueError(f"avg.decay must be a number in [0, 1], got {decay!r}")
    every = values.get("every", 1)
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError(f"avg.every must be an integer >= 1, got {every!r}")
    start = values.get("start_epoch", 0)
    if isinstance(start, bool) or not isinstance(start, int) or start < 0:
        raise ValueError(f"avg.start_epoch must be an integer >= 0, got {start!r}")
    buffers = values.get("buffers", "copy")
    if buffers not in BUFFERS:
        raise ValueError(f"avg.buffers must be copy or average, got {buffers!r}")
    select = values.get("select", "model")
    if select not in ("model", "averaged"):
        raise ValueError(f"avg.select must be model or averaged, got {select!r}")
    bn = _on_off(values.get("update_bn", False), "update_bn")
    if kind == "off":
        return None
    return Options(kind, float(decay), every, start, buffers, select, bn)


def build(cfg, model):
    """(Options, AveragedModel over `model`) of the config's `avg:` block, (None, None) without one."""
    opts = options(cfg)
    if opts is None:
        return None, None
    return opts, AveragedModel(model, kind=opts.kind, decay=opts.decay, buffers=opts.buffers)

"""PROSER (Zhou, Ye, Zhan, "Learning Placeholders for Open-Set Recognition", CVPR 2021) on the MI355X: a short fine-tuning stage that
turns a trained closed-set network into an open-set classifier by reserving placeholders for the unknown.

    proser = PROSER(model, dummy_count=5, mix_at="layer3")      # model: a trained ResNet50 on the device
    opt_model = optim.SGD(model, lr=1e-3)                        # the fused optimizers, over the trainable suffix
    opt_dummy = torch.optim.SGD(proser.dummy_classifier.parameters(), lr=1e-3)
    for epoch in range(epochs):
        proser.train_epoch(loader, opt_model, opt_dummy, trackers)
    proser.fit_bias(val_logits, val_dummy, val_gt)               # arrays of the validation split
    probs = proser.predict(logits, dummy)                        # [M, C + 1] fp32 on the device, the unknown column LAST

Every step mixes the first half of the batch pairwise in the middle of the network (manifold mixup: ResNet50.next_forward(mix=...)), adds
a small "dummy" classifier on the deep features and trains the suffix and the dummy classifier with a three-term cross-entropy over
[logits, max dummy]: mixed rows belong to the placeholder, clean rows to their class, and clean rows with their class taken out to the
placeholder again. The method is not part of the reference snapshot: include/osi.h (ABI 23) is its definition,
tests/proser_oracle.py its fp64 restatement.

Properties of this build, by design:
  * the mix lives at the cut of `freeze_below(mix_at)`: stem and layers below `mix_at` are frozen entirely (weights and statistics) for
    the stage, the backward ends at the cut and no gradient crosses the mix. Full-depth mixing is out of scope;
  * the model's parameters live in the arena and take the fused optimizers (openset_imagenet.optim); the two tensors of the dummy
    classifier live outside it and take a torch.optim optimizer of the caller's;
  * pairs are drawn regardless of label (no same-class rejection); single GPU (the dummy gradients are not all-reduced); no
    worker() integration, no AveragedModel.
All arithmetic runs in the kernels of csrc/proser.hip and csrc/linear.hip (torch.ops.osi.*); there is no CPU path.
"""
import math

import numpy as np
import torch
from torch import nn

from . import _native as N
from .model import ResNet50
from .util import _labels_on_device, _need_gpu

_SETTINGS = ("dummy_count", "mix_at", "lambdas", "alpha")


class _LinearFn(torch.autograd.Function):
    """y = x w^T + b on the package's own dense kernels (osi_linear_fwd / osi_linear_bwd): no vendor GEMM."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        return N.ops().linear_fwd(x, w.contiguous(), b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx, dw, db = N.ops().linear_bwd(dy.contiguous(), x, w.contiguous(), bool(ctx.needs_input_grad[0]))
        return (dx if ctx.needs_input_grad[0] else None), dw, db


class ProserLoss(torch.autograd.Function):
    """The three-term loss of osi_proser_loss_fwd_bwd: `ProserLoss.apply(logits, dummy, target, n_mixed, lambdas)` returns
    (J, terms) with terms = [J, mean t1, mean t2, mean t3] (not differentiable). The gradients were computed by the forward launch."""

    @staticmethod
    def forward(ctx, logits, dummy, target, n_mixed, lambdas):
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        l0, l1, l2 = lambdas
        loss4, dlogits, ddummy = N.ops().proser_loss_fwd_bwd(logits.contiguous(), dummy.contiguous(), target.contiguous(), int(n_mixed),
                                                             float(l0), float(l1), float(l2), bool(need_grad))
        ctx.save_for_backward(dlogits, ddummy)
        ctx.mark_non_differentiable(loss4)
        return loss4[0].clone(), loss4

    @staticmethod
    def backward(ctx, grad_out, _):
        dlogits, ddummy = ctx.saved_tensors
        return dlogits * grad_out, ddummy * grad_out, None, None, None


def _check_rows(logits, dummy, what):
    l_shape, d_shape = tuple(torch.as_tensor(logits).shape), tuple(torch.as_tensor(dummy).shape)
    if len(l_shape) != 2 or len(d_shape) != 2:
        raise ValueError(f"{what}: logits and dummy must be matrices [M, C] and [M, D], got shapes {l_shape} and {d_shape}")
    if l_shape[0] != d_shape[0]:
        raise ValueError(f"{what}: logits and dummy disagree on the number of samples: {l_shape[0]} and {d_shape[0]}")
    if l_shape[1] == 0 or d_shape[1] == 0:
        raise ValueError(f"{what}: logits and dummy must have at least one column, got shapes {l_shape} and {d_shape}")
    return l_shape, d_shape


def _f32(x, dev):
    return torch.as_tensor(x).detach().to(device=dev, dtype=torch.float32).contiguous()


def bias_index(n, known_rate):
    """0-based rank of the calibrated bias among the n ascending differences: floor((1 - known_rate) * n), at most n - 1."""
    return min(int(math.floor((1.0 - known_rate) * n)), n - 1)


class PROSER(nn.Module):
    def __init__(self, model, dummy_count=5, mix_at="layer3", lambdas=(0.01, 1.0, 1.0), alpha=1.0, generator=None):
        super().__init__()
        if not isinstance(model, ResNet50):
            raise TypeError(f"model must be an openset_imagenet.ResNet50, got {type(model).__name__}")
        if isinstance(dummy_count, bool) or not isinstance(dummy_count, int):
            raise TypeError(f"dummy_count must be an int, got {type(dummy_count).__name__}")
        if dummy_count < 1:
            raise ValueError(f"dummy_count must be >= 1, got {dummy_count}")
        try:
            lambdas = tuple(float(v) for v in lambdas)
        except (TypeError, ValueError):
            raise TypeError("lambdas must be three numbers (the factors of the mixed, the clean and the left-out term)") from None
        if len(lambdas) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in lambdas):
            raise ValueError(f"lambdas must be three finite numbers >= 0, got {lambdas}")
        alpha = float(alpha)
        if not (math.isfinite(alpha) and alpha > 0.0):
            raise ValueError(f"alpha (the Beta(alpha, alpha) of the mixing weight) must be finite and > 0, got {alpha}")
        if generator is not None and not isinstance(generator, np.random.Generator):
            raise TypeError(f"generator must be a numpy.random.Generator or None, got {type(generator).__name__}")
        unit = model._unit_of(mix_at)         # ValueError for a name that is no cut
        if unit == model._n_units - 1:
            raise ValueError("mix_at must name a block ('layer1' .. 'layer4' or 'layerN.K'): the mix needs a block input, 'fc' has none")
        self.model = model
        self.dummy_count, self.mix_at, self.lambdas, self.alpha = dummy_count, mix_at, lambdas, alpha
        self.generator = generator if generator is not None else np.random.default_rng()
        model.freeze_below(mix_at)
        dev = model.flat_parameters().device
        self.dummy_classifier = nn.Linear(model._F, dummy_count).to(dev)    # torch's Linear initialisation
        self.register_buffer("bias", torch.zeros((), dtype=torch.float32, device=dev))
        self.terms = None        # [J, mean t1, mean t2, mean t3] of the latest training_step, on the device

    # ------------------------------------------------------------------------------------------------------------ forward
    def forward(self, images):
        """(logits [B, C], dummy [B, D], features [B, F]); a pending ResNet50.next_forward request applies to the model's forward."""
        logits, features = self.model(images)
        dummy = _LinearFn.apply(features, self.dummy_classifier.weight, self.dummy_classifier.bias)
        return logits, dummy, features

    def dummy_logits(self, features):
        """[M, D] fp32 on the device: the dummy classifier on deep features [M, F] (numpy or torch, host or device), without a graph."""
        f_shape = tuple(torch.as_tensor(features).shape)
        if len(f_shape) != 2 or f_shape[1] != self.dummy_classifier.in_features:
            raise ValueError(f"features must be [M, {self.dummy_classifier.in_features}], got shape {f_shape}")
        dev = _need_gpu("PROSER.dummy_logits")
        if f_shape[0] == 0:
            return torch.empty(0, self.dummy_count, dtype=torch.float32, device=dev)
        with torch.no_grad():
            return N.ops().linear_fwd(_f32(features, dev), _f32(self.dummy_classifier.weight, dev), _f32(self.dummy_classifier.bias, dev))

    def draw_pairs(self, B):
        """(partner int32 [B], weight fp32 [B], n_mixed) as host numpy arrays: a uniformly random perfect matching of the rows
        [0, n_mixed), n_mixed = (B // 2) & ~1, with ONE lam ~ Beta(alpha, alpha) for the step; the rows from n_mixed on are their own
        partners with weight 1. Pairs are drawn regardless of label."""
        if isinstance(B, bool) or not isinstance(B, (int, np.integer)):
            raise TypeError(f"B must be an int, got {type(B).__name__}")
        if B < 1:
            raise ValueError(f"B must be >= 1, got {B}")
        n_mixed = (int(B) // 2) & ~1
        partner = np.arange(B, dtype=np.int32)
        weight = np.ones(B, dtype=np.float32)
        perm = self.generator.permutation(n_mixed)          # consecutive entries of a uniform permutation: a uniform perfect matching
        lam = self.generator.beta(self.alpha, self.alpha)
        partner[perm[0::2]] = perm[1::2]
        partner[perm[1::2]] = perm[0::2]
        weight[:n_mixed] = lam
        return partner, weight, n_mixed

    def training_step(self, images, labels):
        """Draw the pairs, run the mixed forward and the loss; returns the loss J (0-dim, `.backward()` goes through autograd: dlogits to
        the backbone's node, ddummy to the dummy classifier, whose backward adds dfeatures). self.terms holds the four loss values."""
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
            raise TypeError("labels must be an int64 tensor [B]")
        if labels.dim() != 1 or not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[0] != labels.shape[0]:
            raise ValueError("images must be a batch of B images and labels a vector of B entries")
        dev = self.model.flat_parameters().device
        if dev.type != "cuda" or not labels.is_cuda:
            raise RuntimeError("openset_imagenet (MI355X build) has no CPU path: PROSER.training_step needs the model, the batch and the "
                               "labels on the GPU")
        B = labels.shape[0]
        partner, weight, n_mixed = self.draw_pairs(B)
        # built on the host, copied without a sync
        self.model.next_forward(mix=(torch.from_numpy(partner).to(dev, non_blocking=True), torch.from_numpy(weight).to(dev, non_blocking=True)))
        logits, dummy, _ = self(images)
        j, self.terms = ProserLoss.apply(logits, dummy, labels, n_mixed, self.lambdas)
        return j

    def train_epoch(self, loader, opt_model, opt_dummy, trackers=None):
        """One epoch of the stage. opt_model: a fused optimizer (openset_imagenet.optim) over the model; opt_dummy: a torch.optim
        optimizer over dummy_classifier.parameters() (they live outside the arena). trackers["j"] (optional, an AverageMeter) receives
        every batch's loss at the end of the epoch: nothing is read back inside it."""
        from .pipeline import device_batch
        if trackers:
            for metric in trackers.values():
                metric.reset()
        pending, counts = [], []
        self.model.train()
        self.dummy_classifier.train()
        for batch in loader:
            images, labels = device_batch(batch)
            opt_model.zero_grad()
            opt_dummy.zero_grad()
            j = self.training_step(images, labels)
            j.backward()
            opt_model.step()
            opt_dummy.step()
            pending.append(j.detach())
            counts.append(labels.shape[0])
        if pending and trackers and "j" in trackers:
            for value, n in zip(torch.stack(pending).cpu().tolist(), counts):
                trackers["j"].update(value, n)

    # -------------------------------------------------------------------------------------------------------- calibration
    def fit_bias(self, logits, dummy, gt, known_rate=0.95):
        """Calibrate `bias` on the validation split: over the rows with 0 <= gt < C, delta = max_c logits - max_d dummy (on the device);
        bias becomes the floor((1 - known_rate) * n)-th smallest delta (0-based), so about known_rate of the known rows keep a class
        logit above the placeholder's. Returns self."""
        known_rate = float(known_rate)
        if not 0.0 < known_rate <= 1.0:
            raise ValueError(f"known_rate must lie in (0, 1], got {known_rate!r}")
        l_shape, _ = _check_rows(logits, dummy, "fit_bias")
        if len(gt) != l_shape[0]:
            raise ValueError(f"fit_bias: logits and gt disagree on the number of samples: {l_shape[0]} and {len(gt)}")
        dev = _need_gpu("PROSER.fit_bias")
        lg, dm, y = _f32(logits, dev), _f32(dummy, dev), _labels_on_device(gt, dev)
        known = (y >= 0) & (y < l_shape[1])
        delta = (lg.max(dim=1).values - dm.max(dim=1).values)[known]
        n = int(delta.numel())
        if n == 0:
            raise ValueError("fit_bias: gt holds no label inside [0, C): there is no known row to calibrate on")
        self.bias = torch.sort(delta).values[bias_index(n, known_rate)].to(self.bias.device).clone()
        return self

    def predict(self, logits, dummy):
        """[M, C + 1] fp32 on the device: softmax([logits, max_d dummy + bias]), the unknown class in the LAST column."""
        l_shape, _ = _check_rows(logits, dummy, "predict")
        dev = _need_gpu("PROSER.predict")
        if l_shape[0] == 0:
            return torch.empty(0, l_shape[1] + 1, dtype=torch.float32, device=dev)
        return N.ops().proser_scores(_f32(logits, dev), _f32(dummy, dev), float(self.bias))

    # -------------------------------------------------------------------------------------------------------------- state
    def state_dict(self, *args, **kwargs):
        """model.*, dummy_classifier.*, bias, and the settings (dummy_count, mix_at, lambdas, alpha) as plain values."""
        sd = super().state_dict(*args, **kwargs)
        prefix = kwargs.get("prefix", args[1] if len(args) > 1 else "")
        for name in _SETTINGS:
            sd[prefix + name] = getattr(self, name)
        return sd

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        sd = dict(state_dict)
        missing = [k for k in _SETTINGS if k not in sd]
        if missing:
            raise ValueError(f"state dict lacks {missing}")
        settings = {k: sd.pop(k) for k in _SETTINGS}
        if int(settings["dummy_count"]) != self.dummy_count:
            raise ValueError(f"state dict: dummy_count is {settings['dummy_count']}, this module was built with {self.dummy_count}")
        out = super().load_state_dict(sd, strict=strict, **kwargs)
        self.mix_at, self.alpha = settings["mix_at"], float(settings["alpha"])
        self.lambdas = tuple(float(v) for v in settings["lambdas"])
        self.model.freeze_below(self.mix_at)
        return out

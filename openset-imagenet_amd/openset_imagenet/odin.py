"""Gradient-based open-set scores on the MI355X: ODIN (Liang, Li, Srikant, "Enhancing The Reliability of Out-of-distribution Image
Detection in Neural Networks", ICLR 2018) and GradNorm (Huang, Geng, Li, "On the Importance of Gradients for Detecting Distributional
Shifts in the Wild", NeurIPS 2021). Unlike the other post-hoc detectors of this package ODIN touches the image: it scores the
temperature-scaled largest softmax probability after one signed-gradient step on the input,

    S_c(x; T) = softmax(logits(x) / T)_c,   y = argmax_c logits(x),   J = -log S_y(x; T)
    x~ = clamp(x - epsilon * sign(dJ/dx), lo, hi)            the step RAISES the predicted class's probability
    unknown = -max_c S_c(x~; T)                               higher = more unknown, as `--detection` expects

    odin = ODIN(temperature=1000.0, epsilon=0.0014)
    dlogits, pred, score = odin.head(logits)                 # the kernel: the seed of the backward, torch.argmax, S_y(x; T)
    logits, features, x_t = odin.perturb(model, images)      # the clean forward's outputs and x~
    out = odin.scores(model, images)                         # logits, features, scores (clean softmax), logits_odin, unknown
    arr = odin.arrays(model, loader)                         # the same over a loader, numpy, with gt
    odin.tune(model, loader, temperatures, epsilons)         # the paper's grid search on a split with negatives (label -1)
    g = gradnorm_scores(features, logits, temperature=1.0)   # [M]: GradNorm for the last linear layer, higher = more known

The defaults are the paper's values, taken in THIS network's pixel units: the network is fed ToTensor() output in [0, 1] without a
per-channel normalisation, so epsilon is a step in [0, 1] pixels and is not divided by a channel's standard deviation. Nothing here
claims these values are good for this network: tune them.

On the MI355X ResNet50 (also wrapped for data parallel) a batch costs one differentiable forward on the running statistics, one
INPUT-ONLY backward and one inference forward: the backward is seeded with the head's dlogits = d(T J)/dlogits (osi_odin_head,
include/osi.h ABI 29: T times the textbook gradient, so that the seed's magnitude does not depend on T - only the sign of dJ/dx is
used) and ends in the projected step of the stem kernel with alpha = -epsilon (ResNet50.next_backward(pgd=(-epsilon, inf, None),
input_only=True)): dJ/dx is never written, no parameter gradient is computed, and the running statistics, num_batches_tracked, every
p.grad, the gradient arena, its "fresh" mark and the optimizers' state stay as they are. NCHW fp32, NHWC4 and uint8 [B, H, W, 3]
batches are served alike; x~ is adversarial_batch() (NHWC4, model-owned). The model's mode is restored afterwards, also on an
exception. Any other torch model that returns (logits, features) goes through autograd w.r.t. the image and adversary.pgd_step, with
the head restated in torch in the tensor's dtype (the only arithmetic here that is not a kernel), so that route also runs on the CPU.

tune() runs, per batch and temperature, one differentiable forward and one input-only backward through the dJ/dimage route (the sign
of dJ/dx depends on T and not on epsilon) and builds x~ for every epsilon with adversary.pgd_step: |T| backwards and |T| * |epsilon|
inference forwards per batch. It selects the lowest FPR at 95 % TPR of the known rows against the rows labelled `unk_label`
(metrics.detection_metrics), ties by the higher AUROC, then the smaller T, then the smaller epsilon.

GradNorm's score ||f||_1 * sum_c |C p_c - 1| / T, p = softmax(logits / T), is the L1 norm of d/dW sum_c -log p_c for logits = W f (the
paper's loss with the all-ones target; a bias does not enter): one kernel on (features, logits).

Out of scope: input preprocessing for other scores (Mahalanobis' variant, an energy seed; ODIN._seed is the one place a seed is made),
Generalized ODIN, GradNorm w.r.t. any layer but the last, ODIN through a freeze_below prefix (refused), multi-GPU arrays / tune."""
import math

import numpy as np
import torch

from . import _native as N
from . import metrics
from ._detector import Detector, _matrix
from .adversary import _mi355x_net, as_nhwc4, pgd_step
from .util import _need_gpu

GRID_COLUMNS = ("temperature", "epsilon", "fpr_at_tpr95", "auroc", "aupr_in", "aupr_out")


def _number(value, name, positive):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {value!r}")
    value = float(value)
    if not math.isfinite(value) or (value <= 0.0 if positive else value < 0.0):
        raise ValueError(f"{name} must be finite and {'> 0' if positive else '>= 0'}, got {value}")
    return value


def _numbers(values, name, positive):
    try:
        values = list(values)
    except TypeError:
        raise ValueError(f"{name} must be a sequence of numbers, got {values!r}") from None
    if not values:
        raise ValueError(f"{name} must not be empty")
    return [_number(v, f"{name}[{i}]", positive) for i, v in enumerate(values)]


def head_reference(logits, temperature, need_grad=True):
    """(dlogits or None, pred, score) of osi_odin_head (include/osi.h, ABI 29) restated with torch ops in the dtype of `logits`, on
    whatever device they live: the head of the route for models other than the MI355X ResNet50."""
    z = logits.detach()
    if z.dim() != 2 or z.shape[1] == 0:
        raise ValueError(f"logits must be a matrix [M, C] with C >= 1, got shape {tuple(z.shape)}")
    pred = z.argmax(1)
    m = z.max(1).values
    shift = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp((z - shift[:, None]) / temperature)
    own = torch.zeros_like(z, dtype=torch.bool).scatter_(1, pred[:, None], True)
    e_y = e.gather(1, pred[:, None])[:, 0]
    r = torch.where(own, torch.zeros_like(e), e).sum(1)
    s = e_y + r
    score = e_y / s
    if not need_grad:
        return None, pred, score
    return torch.where(own, (-r / s)[:, None].expand_as(e), e / s[:, None]), pred, score


def gradnorm_scores(features, logits, temperature=1.0):
    """[M] fp32 on the device: ||f||_1 * sum_c |C p_c - 1| / T with p = softmax(logits / T) (osi_gradnorm_scores; higher = more
    known). features [M, F] and logits [M, C]: numpy arrays or torch tensors, on the host or on the device."""
    temperature = _number(temperature, "temperature", True)
    f_shape, l_shape = tuple(torch.as_tensor(features).shape), tuple(torch.as_tensor(logits).shape)
    if len(f_shape) != 2 or len(l_shape) != 2 or f_shape[0] != l_shape[0] or 0 in f_shape or 0 in l_shape:
        raise ValueError(f"features [M, F] and logits [M, C] must be non-empty matrices of one row count, got shapes {f_shape}, {l_shape}")
    dev = _need_gpu("gradnorm_scores")
    return N.ops().gradnorm_scores(_matrix(features, dev, "features"), _matrix(logits, dev, "logits"), temperature)


class _eval_mode:
    """eval mode for the duration; the mode found is restored on the way out, also on an exception, and no request of the MI355X
    ResNet50 stays pending after one (the pattern of adversary._pgd_steps)."""

    def __init__(self, model, net):
        self.model, self.net = model, net
        self.module = model if net is None else net

    def __enter__(self):
        self.was_training = self.module.training
        self.model.eval()

    def __exit__(self, kind, *exc):
        if kind is not None and self.net is not None:
            self.net._bw_request = None       # a request whose backward never ran must not reach a later one
        self.model.train(self.was_training)
        return False


class _frozen_parameters:
    """requires_grad off on every parameter for the duration (the flags found are put back): what makes a backward through the
    dJ/dimage route input-only. No p.grad is touched."""

    def __init__(self, module):
        self.params = [p for p in module.parameters() if p.requires_grad]

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


class ODIN(Detector):
    _STATE = ("grid",)             # [G, 6] fp64, the rows of GRID_COLUMNS for every grid point of tune(); G = 0 before any tune
    _SETTINGS = ("temperature", "epsilon", "lo", "hi")
    _DTYPES = {"grid": torch.float64}
    _FIT = "tune(model, loader, temperatures, epsilons)"

    def __init__(self, temperature=1000.0, epsilon=0.0014, lo=0.0, hi=1.0):
        self.temperature = _number(temperature, "temperature", True)
        self.epsilon = _number(epsilon, "epsilon", False)
        for name, v in (("lo", lo), ("hi", hi)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or math.isnan(float(v)):
                raise ValueError(f"{name} must be a number, got {v!r}")
        self.lo, self.hi = float(lo), float(hi)
        if not self.lo <= self.hi:
            raise ValueError(f"lo <= hi is needed, got lo = {self.lo}, hi = {self.hi}")
        self.grid = torch.zeros(0, len(GRID_COLUMNS), dtype=torch.float64)
        self._ws = None

    # --------------------------------------------------------------------------------------------------------------- head
    def head(self, logits):
        """(dlogits [M, C], pred [M] int64, score [M]) of osi_odin_head at this temperature, fp32 on the device."""
        shape = tuple(torch.as_tensor(logits).shape)
        if len(shape) != 2 or 0 in shape:
            raise ValueError(f"logits must be a non-empty matrix [M, C], got shape {shape}")
        dev = _need_gpu("ODIN.head")
        return tuple(N.ops().odin_head(_matrix(logits, dev, "logits"), self.temperature, True))

    @staticmethod
    def _head(logits, temperature, kernel, need_grad):
        if kernel:
            dlogits, pred, score = N.ops().odin_head(logits.detach().contiguous(), temperature, need_grad)
            return (dlogits if need_grad else None), pred, score
        return head_reference(logits, temperature, need_grad)

    def _seed(self, logits, features, temperature, kernel):
        """The gradient the backward starts from, (dlogits, dfeatures): ODIN's is d(T J)/dlogits of J = -log S_y(x; T) and nothing on
        the features. The one place a seed is made."""
        return self._head(logits, temperature, kernel, True)[0], None

    # ------------------------------------------------------------------------------------------------------------ perturb
    @staticmethod
    def _route(model):
        net = _mi355x_net(model)
        if net is not None and net.frozen_below is not None:
            raise ValueError(f"ODIN needs the image gradient through the whole network and cannot be combined with freeze_below "
                             f"({net.frozen_below!r} is declared): there is no image gradient behind an inference-form prefix; clear the "
                             "declaration with freeze_below(None)")
        return net

    def _perturb(self, model, net, images):
        """perturb() inside _eval_mode."""
        with torch.enable_grad():
            if net is not None:
                net.next_backward(pgd=(-self.epsilon, math.inf, None), lo=self.lo, hi=self.hi, input_only=True)
                logits, features = model(images)
                dlogits, _ = self._seed(logits, features, self.temperature, True)
                logits.backward(dlogits)
                return logits.detach(), features.detach(), net.adversarial_batch()
            xi = images.detach().requires_grad_()
            logits, features = model(xi)
            dlogits, _ = self._seed(logits, features, self.temperature, False)
            grad, = torch.autograd.grad(logits, xi, dlogits)
            x = xi.detach()
            return logits.detach(), features.detach(), pgd_step(x, grad, x, -self.epsilon, math.inf, self.lo, self.hi)

    def perturb(self, model, images):
        """(clean logits, clean features, x~) with x~ = clamp(x - epsilon * sign(dJ/dx), lo, hi): NHWC4 (model-owned,
        ResNet50.adversarial_batch()) on the MI355X ResNet50, in the layout of `images` on any other model."""
        net = self._route(model)
        with _eval_mode(model, net):
            return self._perturb(model, net, images)

    def scores(self, model, images):
        """dict of device tensors: `logits`, `features` (the clean forward's), `scores` (the clean row softmax: the closed-set decision
        stays the network's), `logits_odin` (a no-grad inference forward on x~) and `unknown` = -max_c S_c(x~; T) [B]."""
        net = self._route(model)
        with _eval_mode(model, net):
            logits, features, x_t = self._perturb(model, net, images)
            with torch.no_grad():
                logits_odin, _ = model(x_t)
                score = self._head(logits_odin, self.temperature, net is not None, False)[2]
                scores = N.ops().softmax(logits.contiguous()) if net is not None else torch.softmax(logits, 1)
        return dict(logits=logits, features=features, scores=scores, logits_odin=logits_odin.detach(), unknown=-score)

    @staticmethod
    def _batch(net, batch):
        if net is None:
            images, labels = batch
            return images, labels
        from .pipeline import device_batch
        return device_batch(batch)

    def arrays(self, model, loader):
        """scores() over a loader (pipeline.device_batch takes its batches): `gt` (float32, as train.get_arrays writes it), `logits`,
        `features`, `scores`, `logits_odin`, `unknown` as numpy arrays, gathered on the device and copied out once."""
        net = self._route(model)
        keys = ("logits", "features", "scores", "logits_odin", "unknown")
        parts = {k: [] for k in ("gt",) + keys}
        for batch in loader:
            images, labels = self._batch(net, batch)
            out = self.scores(model, images)
            parts["gt"].append(torch.as_tensor(labels).to(out["unknown"].device))
            for k in keys:
                parts[k].append(out[k])
        if not parts["gt"]:
            raise ValueError("ODIN.arrays: the loader is empty")
        arrays = {k: torch.cat(v).cpu().numpy() for k, v in parts.items()}
        arrays["gt"] = arrays["gt"].astype(np.float32)
        return arrays

    # --------------------------------------------------------------------------------------------------------------- tune
    def _image_grad(self, model, net, x, temperature):
        """dJ/dx [B, 3, H, W] (up to the positive factor of the seed) of the NCHW batch x at `temperature`: one differentiable
        forward, one input-only backward."""
        with torch.enable_grad():
            xi = x.detach().requires_grad_()
            if net is not None:
                with _frozen_parameters(net):         # no parameter requires grad: the dJ/dimage route computes dJ/dimage alone
                    logits, features = model(xi)
                    dlogits, _ = self._seed(logits, features, temperature, True)
                    grad, = torch.autograd.grad(logits, xi, dlogits)
            else:
                logits, features = model(xi)
                dlogits, _ = self._seed(logits, features, temperature, False)
                grad, = torch.autograd.grad(logits, xi, dlogits)
        return grad

    @staticmethod
    def select(grid):
        """The row of `grid` ([G, 6], GRID_COLUMNS) tune() picks: the lowest FPR at 95 % TPR, ties by the higher AUROC, then the smaller
        temperature, then the smaller epsilon."""
        rows = np.asarray(grid, dtype=np.float64)
        return min(range(len(rows)), key=lambda i: (rows[i][2], -rows[i][3], rows[i][0], rows[i][1]))

    def tune(self, model, loader, temperatures, epsilons, unk_label=-1):
        """Grid search over temperatures x epsilons on a split with negatives (see the module docstring); sets `temperature` and
        `epsilon` to the selected point, keeps every point's figures in `grid` ([G, 6] fp64, GRID_COLUMNS, temperature-major) and
        returns self. ValueError when the split has no row labelled `unk_label`, or no known row."""
        temperatures, epsilons = _numbers(temperatures, "temperatures", True), _numbers(epsilons, "epsilons", False)
        if isinstance(unk_label, bool) or not isinstance(unk_label, (int, np.integer)) or unk_label >= 0:
            raise ValueError(f"unk_label must be a negative integer, got {unk_label!r}")
        net = self._route(model)
        gt, unknown = [], [[[] for _ in epsilons] for _ in temperatures]
        with _eval_mode(model, net):
            for batch in loader:
                images, labels = self._batch(net, batch)
                x = images.detach() if net is None else as_nhwc4(images)[..., :3].permute(0, 3, 1, 2).contiguous()
                gt.append(torch.as_tensor(labels))
                for ti, temperature in enumerate(temperatures):
                    grad = self._image_grad(model, net, x, temperature)
                    for ei, epsilon in enumerate(epsilons):
                        with torch.no_grad():
                            logits_odin, _ = model(pgd_step(x, grad, x, -epsilon, math.inf, self.lo, self.hi))
                            unknown[ti][ei].append(-self._head(logits_odin, temperature, net is not None, False)[2])
        if not gt:
            raise ValueError("ODIN.tune: the loader is empty")
        gt = torch.cat([g.cpu() for g in gt]).numpy().astype(np.int64)
        if not (gt == unk_label).any():
            raise ValueError(f"ODIN.tune: the split has no row labelled {unk_label}: there is nothing to tell the known rows from")
        if not (gt >= 0).any():
            raise ValueError("ODIN.tune: the split has no known row (every label is negative)")
        rows = []
        for ti, temperature in enumerate(temperatures):
            for ei, epsilon in enumerate(epsilons):
                m = metrics.detection_metrics(gt, torch.cat(unknown[ti][ei]).cpu().numpy(), unk_label=int(unk_label), tpr=(0.95,))
                rows.append([temperature, epsilon, m["fpr_at_tpr"][0], m["auroc"], m["aupr_in"], m["aupr_out"]])
        self.grid = torch.tensor(rows, dtype=torch.float64)
        self.temperature, self.epsilon = rows[self.select(rows)][:2]
        return self

    # -------------------------------------------------------------------------------------------------------------- state
    def _restore(self, sd, t):
        grid = t["grid"]
        if grid.dim() != 2 or grid.shape[1] != len(GRID_COLUMNS):
            raise ValueError(f"state dict: grid must be [G, {len(GRID_COLUMNS)}], got shape {tuple(grid.shape)}")
        ODIN.__init__(self, sd["temperature"], sd["epsilon"], sd["lo"], sd["hi"])

"""Activation shaping on the MI355X: ReAct (Sun, Guo, Li, "ReAct: Out-of-distribution Detection With Rectified Activations", NeurIPS
2021), ASH-P / ASH-B / ASH-S (Djurisic, Bozanic, Ashok, Liu, "Extremely Simple Activation Shaping for Out-of-Distribution Detection",
ICLR 2023) and SCALE (Xu, Chen, Fang, Wang, Pan, "Scaling for Training Time and Post-hoc Out-of-distribution Detection Enhancement",
ICLR 2024), scored with the energy of the re-computed logits (Liu, Wang, Owens, Li, "Energy-based Out-of-distribution Detection",
NeurIPS 2020). The methods rectify, prune or rescale the network's penultimate activation - the non-negative [B, 2048] average-pooled
output of layer4 (ResNet50.pooled(), train.get_arrays(pooled=True)) -, push it through the two head layers again and read the log-sum-exp.

    head = head_of(model)                          # (fc_weight [F, P], fc_bias [F], logit_weight [C, F], logit_bias [C] or None)
    s = ActivationShaping("react")                 # or "ash_p", "ash_b", "ash_s", "scale"; percentile=None takes the default below
    s.fit(pooled, gt, head=head)                   # react: the clip is the percentile of the TRAINING split's pooled activations
                                                   # (rows with gt < 0 are ignored); the others need no data: fit(None, head=head)
    x = s.shape(pooled)                            # [M, P] fp32 on the device: the shaped activation
    lg = s.logits(pooled)                          # [M, C]: fc, then the logit layer, on the shaped activation (ops.linear_fwd twice)
    unknown = s.unknown_score(pooled)              # [M]: -logsumexp(lg) (larger = more unknown, the sign convention of ViM)
    scores = s.predict(pooled)                     # [M, C]: softmax(lg) (larger = more known)
    s.energy(pooled), s.max_logit(pooled), s.msp(pooled)     # [M]: logsumexp, largest logit, largest softmax probability of lg

react clips every activation at `clip`, the `percentile`-th percentile (numpy's `linear` rule) of all pooled activations of the counted
training rows: two exact order statistics from the device (osi_order_stats_f32, one read-back), interpolated in fp64 on the host. The
others keep, per row, the keep(P) = P - round(P * percentile / 100) largest activations (the rule of the ASH code; ties by the lowest
column): ash_p zeroes the rest, ash_b also replaces the kept ones by (row sum) / keep, ash_s also multiplies them by exp(s1 / s2) with
s1 the row sum and s2 the sum of the kept ones, scale multiplies the WHOLE row by that factor and prunes nothing. An all-zero row gives
0 / 0 under ash_s and scale: its shaped activation, logits and scores are NaN, as the formula says (include/osi.h, ABI 27).

The default percentiles - react 90, ash_p 60, ash_b 65, ash_s 90, scale 85 - are the ResNet-50 / ImageNet settings of the papers as
remembered; they have NOT been verified against the papers' code, and nothing depends on them: pass `percentile`.

Everything runs in the kernels of csrc/shaping.hip and csrc/linear.hip; there is no CPU path. Inputs may be numpy arrays or torch
tensors, on the host or on the device. Rows go through the kernels in the pieces of _detector._launch_rows, or of `chunk=` rows. The
methods are not part of the reference snapshot: include/osi.h (ABI 27) is their definition, tests/shaping_oracle.py the numpy
restatement. Out of scope: DICE and other weight-masking methods, shaping the un-pooled 7x7 map, P > 4096, multi-GPU fits."""
import math

import numpy as np
import torch

from . import _native as N
from ._detector import Detector, _check_chunk, _launch_rows, _matrix
from .util import _labels_on_device, _need_gpu

METHODS = {"react": N.SHAPE_REACT, "ash_p": N.SHAPE_ASH_P, "ash_b": N.SHAPE_ASH_B, "ash_s": N.SHAPE_ASH_S, "scale": N.SHAPE_SCALE}
DEFAULT_PERCENTILE = {"react": 90.0, "ash_p": 60.0, "ash_b": 65.0, "ash_s": 90.0, "scale": 85.0}      # unverified: see the module docstring


def keep_of(width, percentile):
    """Columns a row of `width` keeps at `percentile`: width - round(width * percentile / 100), the rule of the ASH code; at least 1."""
    k = int(width) - int(np.round(int(width) * percentile / 100.0))
    if k < 1:
        raise ValueError(f"percentile {percentile} keeps {k} of {width} columns; at least 1 must stay")
    return k


def head_of(model):
    """(fc_weight [F, P], fc_bias [F], logit_weight [C, F], logit_bias [C] or None) of a ResNet50: the two layers above the pooled
    activation, detached views of the model's own parameters."""
    named = dict(model.named_parameters())
    try:
        head = named["resnet_base.fc.weight"], named["resnet_base.fc.bias"], named["logits.weight"], named.get("logits.bias")
    except KeyError as e:
        raise TypeError(f"head_of: the model has no parameter {e.args[0]!r}; a ResNet50 is expected") from None
    return tuple(None if t is None else t.detach() for t in head)


def _head_tensors(head):
    """The head as four fp32 host-or-device tensors (the last may be None), shapes checked."""
    if not isinstance(head, (tuple, list)) or len(head) != 4:
        raise TypeError("head must be (fc_weight, fc_bias, logit_weight, logit_bias or None), as head_of(model) returns it")
    if any(t is None for t in head[:3]):
        raise TypeError("head: fc_weight, fc_bias and logit_weight are needed; only logit_bias may be None")
    fw, fb, lw, lb = (None if t is None else torch.as_tensor(t).detach().to(torch.float32).contiguous().clone() for t in head)
    if fw.dim() != 2 or fw.numel() == 0:
        raise ValueError(f"head: fc_weight must be a matrix [F, P], got shape {tuple(fw.shape)}")
    f_dim, p_dim = fw.shape
    if p_dim > N.SHAPE_MAX_F:
        raise ValueError(f"head: the pooled activation is {p_dim} columns wide; the shaping kernels take at most {N.SHAPE_MAX_F}")
    if tuple(fb.shape) != (f_dim,):
        raise ValueError(f"head: fc_bias must be [{f_dim}], got shape {tuple(fb.shape)}")
    if lw.dim() != 2 or lw.shape[0] == 0 or lw.shape[1] != f_dim:
        raise ValueError(f"head: logit_weight must be [C, {f_dim}], got shape {tuple(lw.shape)}")
    if lb is not None and tuple(lb.shape) != (lw.shape[0],):
        raise ValueError(f"head: logit_bias must be [{lw.shape[0]}] or None, got shape {tuple(lb.shape)}")
    return fw, fb, lw, lb


class ActivationShaping(Detector):
    _STATE = ("fc_weight", "fc_bias", "logit_weight")
    _OPTIONAL = ("logit_bias",)
    _SETTINGS = ("method", "percentile", "clip", "count")
    _DTYPES = dict.fromkeys(_STATE + _OPTIONAL, torch.float32)
    _FIT = "fit(pooled, gt, head=head_of(model))"

    def __init__(self, method, percentile=None):
        if not isinstance(method, str):
            raise TypeError(f"method must be one of {sorted(METHODS)}, got {type(method).__name__}")
        if method not in METHODS:
            raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
        if percentile is None:
            percentile = DEFAULT_PERCENTILE[method]
        if isinstance(percentile, bool) or not isinstance(percentile, (int, float, np.integer, np.floating)):
            raise TypeError(f"percentile must be a number or None, got {type(percentile).__name__}")
        percentile = float(percentile)
        if not 0.0 < percentile < 100.0:
            raise ValueError(f"percentile must satisfy 0 < percentile < 100, got {percentile}")
        self.method, self.percentile = method, percentile
        self.clip = self.count = None
        for name in self._STATE + self._OPTIONAL:
            setattr(self, name, None)
        self._ws = None

    # ------------------------------------------------------------------------------------------------------------ helpers
    def keep(self, width):
        """Columns kept of a pooled row of `width`: 0 for react (nothing is pruned), keep_of(width, percentile) otherwise."""
        return 0 if self.method == "react" else keep_of(width, self.percentile)

    def _scratch(self, n, dev):
        lib = N.lib()
        return self._workspace(max(lib.osi_order_stats_workspace(max(n, 1), 2), lib.osi_shape_rows_workspace(1, 1)), dev)

    # ---------------------------------------------------------------------------------------------------------------- fit
    def fit(self, pooled, gt=None, *, head, chunk=None):
        """Keeps `head` (head_of(model)) in fp32. react: `clip` = the percentile of the values of pooled [N, P] over the rows with
        gt >= 0 (gt=None counts every row), `count` = those rows; ValueError when it is not finite. Every other method needs no data:
        pooled may be None, and is only checked for its width when it is given. Returns self."""
        fw, fb, lw, lb = _head_tensors(head)
        p_dim = fw.shape[1]
        _check_chunk(chunk)
        shape = None if pooled is None else tuple(torch.as_tensor(pooled).shape)
        if shape is not None and (len(shape) != 2 or shape[1] != p_dim):
            raise ValueError(f"pooled must be [N, {p_dim}] (the columns of fc_weight), got shape {shape}")
        clip = count = None
        if self.method == "react":
            if shape is None or shape[0] == 0:
                raise ValueError("react needs the pooled activations of the training split: pooled must hold at least one row")
            if gt is not None and len(gt) != shape[0]:
                raise ValueError(f"pooled and gt disagree on the number of samples: {shape[0]}, {len(gt)}")
            if gt is not None and np.ndim(gt) != 1:
                raise ValueError(f"gt must be a vector [N_samples], got shape {tuple(np.shape(gt))}")
            dev = _need_gpu("ActivationShaping.fit")
            x = _matrix(pooled, dev, "pooled")
            if gt is not None:
                x = x[_labels_on_device(gt, dev) >= 0].contiguous()
            count = x.shape[0]
            if count == 0:
                raise ValueError("gt holds no counted row (every label is negative)")
            n = x.numel()
            h = (n - 1) * (self.percentile / 100.0)             # numpy's `linear` rule: the virtual index, its two neighbours
            j = int(math.floor(h))
            a, b = N.ops().order_stats(x, [j, min(j + 1, n - 1)], self._scratch(n, dev)).tolist()     # the one read-back
            clip = a + (h - j) * (b - a)
            if not np.isfinite(clip):
                raise ValueError(f"ActivationShaping.fit: the {self.percentile}-th percentile of the pooled activations, between {a} "
                                 f"and {b}, is not finite")
        else:
            self.keep(p_dim)                                    # refuses a percentile that keeps nothing of this width
        self.fc_weight, self.fc_bias, self.logit_weight, self.logit_bias = fw, fb, lw, lb
        self.clip, self.count = clip, count
        return self

    # ------------------------------------------------------------------------------------------------------------ scoring
    def _pieces(self, pooled, chunk, what, logits):
        """The shaped rows of `pooled`, or their logits, piece by piece: yields (r0, device tensor)."""
        self._require_fit(what)
        p_dim = self.fc_weight.shape[1]
        shape = tuple(torch.as_tensor(pooled).shape)
        if len(shape) != 2 or shape[1] != p_dim:
            raise ValueError(f"pooled must be [M, {p_dim}] (the width fit saw), got shape {shape}")
        _check_chunk(chunk)
        keep = self.keep(p_dim)
        dev = _need_gpu(f"ActivationShaping.{what}")
        self._on(dev)
        m = shape[0]
        if m == 0:
            return
        x = _matrix(pooled, dev, "pooled")
        widest = max(p_dim, self.fc_weight.shape[0], self.logit_weight.shape[0])
        step = min(_launch_rows(m, widest), chunk or m)
        ws = self._scratch(1, dev)
        ops = N.ops()
        clip = 0.0 if self.clip is None else self.clip
        for r0 in range(0, m, step):
            z = ops.shape_rows(x[r0:r0 + step], METHODS[self.method], keep, clip, ws)
            if logits:
                z = ops.linear_fwd(ops.linear_fwd(z, self.fc_weight, self.fc_bias), self.logit_weight, self.logit_bias)
            yield r0, z

    def _gather(self, pooled, chunk, what, columns, piece=None):
        """[M, columns] (or [M] for columns = None) from the logits of every piece, through `piece` where one is given."""
        parts = [z if piece is None else piece(z) for _, z in self._pieces(pooled, chunk, what, logits=what != "shape")]
        if not parts:
            dev = self.fc_weight.device
            return torch.empty((0,) if columns is None else (0, columns), dtype=torch.float32, device=dev)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def shape(self, pooled, chunk=None):
        """[M, P] fp32 on the device: the shaped activation."""
        return self._gather(pooled, chunk, "shape", self.fc_weight.shape[1] if self.is_fitted else 0)

    def logits(self, pooled, chunk=None):
        """[M, C] fp32 on the device: the head on the shaped activation."""
        return self._gather(pooled, chunk, "logits", self.logit_weight.shape[0] if self.is_fitted else 0)

    def predict(self, pooled, chunk=None):
        """[M, C] fp32: the softmax of `logits` (larger = more known)."""
        return self._gather(pooled, chunk, "predict", self.logit_weight.shape[0] if self.is_fitted else 0, N.ops().softmax)

    def _score(self, pooled, chunk, what, mode):
        return self._gather(pooled, chunk, what, None, lambda z: N.ops().logit_scores(z, mode))

    def energy(self, pooled, chunk=None):
        """[M] fp32: logsumexp of `logits` (larger = more known)."""
        return self._score(pooled, chunk, "energy", N.SCORE_ENERGY)

    def max_logit(self, pooled, chunk=None):
        """[M] fp32: the largest of `logits`."""
        return self._score(pooled, chunk, "max_logit", N.SCORE_MAXLOGIT)

    def msp(self, pooled, chunk=None):
        """[M] fp32: the largest softmax probability of `logits`."""
        return self._score(pooled, chunk, "msp", N.SCORE_MSP)

    def unknown_score(self, pooled, chunk=None):
        """[M] fp32: -logsumexp of `logits` (larger = more unknown)."""
        return -self._score(pooled, chunk, "unknown_score", N.SCORE_ENERGY)

    # -------------------------------------------------------------------------------------------------------------- state
    def _restore(self, sd, t):
        fw, fb, lw, lb = _head_tensors((t["fc_weight"], t["fc_bias"], t["logit_weight"], t["logit_bias"]))
        ActivationShaping.__init__(self, sd["method"], sd["percentile"])
        clip = None if sd["clip"] is None else float(sd["clip"])
        if self.method == "react":
            if clip is None or not np.isfinite(clip):
                raise ValueError(f"state dict: react needs a finite clip, got {sd['clip']!r}")
        else:
            self.keep(fw.shape[1])
        self.clip = clip
        self.count = None if sd["count"] is None else int(sd["count"])

"""OpenMax (Bendale & Boult, "Towards Open Set Deep Networks", CVPR 2016) on the MI355X: turn a trained closed-set network into an
open-set classifier after the fact.

    om = OpenMax(tailsize=1000, distance="euclidean", alpha=3)
    om.fit(features, logits, gt)            # the arrays of train.get_arrays on the TRAINING split
    probs = om.predict(logits, features)    # [M, C + 1] fp32 on the device, the unknown column LAST
    w = om.w_scores(features)               # [M, C]

`fit` takes the mean activation vector of every class over its correctly classified rows, measures every such row's distance to
its class mean and fits a Weibull distribution to the `tailsize` largest distances per class; `predict` recalibrates the `alpha`
top-ranked logits of a row by the probability of lying in that tail and appends the activation of the unknown class. The method is
not part of the reference snapshot: include/osi.h (ABI 21) is its definition, tests/openmax_oracle.py its fp64 restatement.
`probs[:, :C]` feeds util.calculate_oscr, util.ccr_at_fpr and util.get_histogram as it is.

All arithmetic runs in the kernels of csrc/openmax.hip (torch.ops.osi.openmax_*); there is no CPU path. Inputs may be numpy arrays
or torch tensors, on the host or on the device. Nothing is read back: `mav`, `shape`, `scale`, `shift`, `fitted`, `count`,
`tail_count` and `flags` ({eligible rows left out for a non-finite distance, unfitted classes}) are device tensors the caller may
read. PROSER is openset_imagenet.proser. Out of scope: per-class tail sizes, multi-GPU fitting.
"""
import torch

from . import _native as N
from ._detector import Detector, _fit_shapes, _matrix
from .util import _labels_on_device, _need_gpu

_METRICS = {"euclidean": N.OPENMAX_EUCLIDEAN, "cosine": N.OPENMAX_COSINE}


class OpenMax(Detector):
    _STATE = ("mav", "shape", "scale", "shift", "fitted", "count", "tail_count", "flags")
    _SETTINGS = ("tailsize", "distance", "alpha")
    _DTYPES = dict(mav=torch.float32, shape=torch.float64, scale=torch.float64, shift=torch.float64, fitted=torch.uint8,
                   count=torch.int64, tail_count=torch.int64, flags=torch.int64)
    _FIT = "fit(features, logits, gt)"

    def __init__(self, tailsize=1000, distance="euclidean", alpha=3):
        if isinstance(tailsize, bool) or not isinstance(tailsize, int):
            raise TypeError(f"tailsize must be an int, got {type(tailsize).__name__}")
        if isinstance(alpha, bool) or not isinstance(alpha, int):
            raise TypeError(f"alpha must be an int, got {type(alpha).__name__}")
        if not 2 <= tailsize <= N.OPENMAX_MAX_TAIL:
            raise ValueError(f"tailsize must lie in [2, {N.OPENMAX_MAX_TAIL}], got {tailsize}")
        if alpha < 1:
            raise ValueError(f"alpha must be >= 1, got {alpha}")
        if distance not in _METRICS:
            raise ValueError(f"distance must be one of {sorted(_METRICS)}, got {distance!r}")
        self.tailsize, self.distance, self.alpha = tailsize, distance, alpha
        for name in self._STATE:
            setattr(self, name, None)
        self._ws = None

    # ---------------------------------------------------------------------------------------------------------------- fit
    def fit(self, features, logits, gt):
        """Class means and Weibull tails from features [N, F], logits [N, C] and labels [N] of the training split. Rows whose label
        lies outside [0, C) (negatives, unknowns) and rows the network classifies wrongly take no part. Returns self."""
        _fit_shapes(features, gt, logits)
        dev = _need_gpu("OpenMax.fit")
        ops = N.ops()
        f, lg, y = _matrix(features, dev, "features"), _matrix(logits, dev, "logits"), _labels_on_device(gt, dev)
        n, c = lg.shape
        ws = self._workspace(N.lib().osi_openmax_workspace(n, c, f.shape[1]), dev)
        self.mav, self.count, correct = ops.openmax_class_means(f, lg, y, ws)
        dist = ops.openmax_distances(f, self.mav, y, _METRICS[self.distance])
        self.shape, self.scale, self.shift, self.fitted, self.tail_count, self.flags = ops.openmax_fit_tails(
            dist, y, correct, c, self.tailsize, ws)
        return self

    # ------------------------------------------------------------------------------------------------------------ predict
    def w_scores(self, features):
        """[M, C] fp32: the probability of every row to lie in the tail of every class (0 for an unfitted class)."""
        self._require_fit("w_scores")
        f_shape = tuple(torch.as_tensor(features).shape)
        if len(f_shape) != 2 or f_shape[1] != self.mav.shape[1]:
            raise ValueError(f"features must be [M, {self.mav.shape[1]}] (the width fit saw), got shape {f_shape}")
        dev = _need_gpu("OpenMax.w_scores")
        self._on(dev)
        ops = N.ops()
        if f_shape[0] == 0:
            return torch.empty(0, self.mav.shape[0], dtype=torch.float32, device=dev)
        dist = ops.openmax_distances(_matrix(features, dev, "features"), self.mav, None, _METRICS[self.distance])
        return ops.openmax_wscores(dist, self.shape, self.scale, self.shift, self.fitted)

    def predict(self, logits, features):
        """[M, C + 1] fp32 on the device: the recalibrated softmax, the unknown class in the LAST column."""
        self._require_fit("predict")
        l_shape, f_shape = tuple(torch.as_tensor(logits).shape), tuple(torch.as_tensor(features).shape)
        c = self.mav.shape[0]
        if len(l_shape) != 2 or l_shape[1] != c:
            raise ValueError(f"logits must be [M, {c}] (the classes fit saw), got shape {l_shape}")
        if len(f_shape) != 2 or f_shape[0] != l_shape[0]:
            raise ValueError(f"features and logits disagree on the number of samples: shapes {f_shape} and {l_shape}")
        w = self.w_scores(features)
        if l_shape[0] == 0:
            return torch.empty(0, c + 1, dtype=torch.float32, device=w.device)
        return N.ops().openmax_recalibrate(_matrix(logits, w.device, "logits"), w, self.alpha)

    # -------------------------------------------------------------------------------------------------------------- state
    def _restore(self, sd, tensors):
        OpenMax.__init__(self, int(sd["tailsize"]), sd["distance"], int(sd["alpha"]))
        if tensors["mav"].dim() != 2:
            raise ValueError(f"state dict: mav must be [C, F], got shape {tuple(tensors['mav'].shape)}")
        c = tensors["mav"].shape[0]
        for k in ("shape", "scale", "shift", "fitted", "count", "tail_count"):
            if tuple(tensors[k].shape) != (c,):
                raise ValueError(f"state dict: {k} must hold one entry per class ({c}), got shape {tuple(tensors[k].shape)}")
        if tuple(tensors["flags"].shape) != (2,):
            raise ValueError(f"state dict: flags must hold two entries, got shape {tuple(tensors['flags'].shape)}")

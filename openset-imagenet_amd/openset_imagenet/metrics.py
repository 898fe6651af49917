"""Validation metrics with the call contract of the reference's openset_imagenet/metrics.py, on the GPU.

  confidence(scores, target_labels, offset=0., unknown_class=-1, last_valid_class=None)     metrics.py:8-42
        -> (kn_conf, kn_count, neg_conf, neg_count); one kernel (osi_confidence_from_scores) instead of boolean-mask indexing
           and Python `sum(known)` loops over device tensors. validate() uses the logits form (osi_confidence_accumulate) and
           never builds the [N_val, C] score matrix at all.
  predict_objectosphere(logits, features, threshold)                                        metrics.py:45-62
        -> [B, 2] tensor (predicted class or -1, max softmax score): softmax on the fused kernel, the rest is three tensor ops.
  auc_score_binary(target_labels, pred_scores, unk_class=-1)                                metrics.py:65-88
  auc_score_multiclass(target_labels, pred_scores)                                          metrics.py:91-106
        -> float: the ROC-AUC that sklearn.metrics.roc_auc_score gives the reference, as the Mann-Whitney quotient of exact pair
           counts made on the device (osi_auc_binary_* / osi_auc_ovr_*, csrc/auc.hip). No sklearn at run time, the [N, C] score
           matrix stays on the device, and the caller's labels are never written (the reference overwrites them with +-1).
"""
import numpy as np
import torch

from . import _native as N
from . import losses as _losses


def confidence(scores, target_labels, offset=0., unknown_class=-1, last_valid_class=None):
    """Model's confidence on known and negative samples (reference metrics.py:8-42); `scores` are softmax scores [N, C]."""
    N.require_gpu_f32(scores, target_labels)
    s = scores.contiguous().float()
    y = target_labels.contiguous().to(torch.int64)
    if last_valid_class == 0:
        raise ValueError("last_valid_class=0 selects no column (scores[:, :0]); use None for all columns")
    acc = torch.zeros(4, dtype=torch.float64, device=s.device)
    N.check(N.lib().osi_confidence_from_scores(N.ptr(s), N.ptr(y), s.shape[0], s.shape[1], float(offset), int(unknown_class),
                                               0 if last_valid_class is None else int(last_valid_class), N.ptr(acc), N.stream_of(s)),
            "osi_confidence_from_scores")
    ks, kc, ns, nc = acc.cpu().tolist()
    return (ks / kc if kc else 0.0), int(kc), (ns / nc if nc else 0.0), int(nc)


def predict_objectosphere(logits, features, threshold):
    """Predicted class (-1 where |f| * max score < threshold) and score (reference metrics.py:45-62)."""
    scores = _losses.softmax(logits)
    pred_score, pred_class = torch.max(scores, dim=1)
    norms = torch.norm(features, p=2, dim=1)
    pred_class = pred_class.clone()
    pred_class[(norms * pred_score) < threshold] = -1
    return torch.stack((pred_class, pred_score), dim=1)


def _auc_inputs(target_labels, pred_scores, what):
    """Labels (int64) and scores (fp32 / fp64 kept, anything else cast to fp64) on the current device, as util.calculate_oscr takes
    them: numpy arrays or torch tensors, host or device. Copies only: the caller's arrays are never written."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"openset_imagenet (MI355X build) has no CPU path: {what} needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.as_tensor(pred_scores).detach()
    if s.dtype not in (torch.float32, torch.float64):
        s = s.double()
    if s.dim() != 2:
        raise ValueError("pred_scores must be [N_samples, N_classes]")
    s = s.to(dev).contiguous()
    y = target_labels.detach() if isinstance(target_labels, torch.Tensor) else torch.as_tensor(np.asarray(target_labels).astype(int))
    y = y.to(torch.int64).to(dev).contiguous()
    if y.numel() != s.shape[0]:
        raise ValueError("target_labels and pred_scores disagree on the number of samples")
    return y, s


def _mann_whitney(gt, eq, pos, neg):
    """(2 gt + eq) / (2 P Nn) on Python ints: one correctly rounded division; nan when a side is empty."""
    return (2 * gt + eq) / (2 * pos * neg) if pos and neg else float("nan")


def _auc_binary_counts(target_labels, pred_scores, unk_class):
    """The device's integers for the binary case: (gt, eq, P, Nn, NaN rows)."""
    y, s = _auc_inputs(target_labels, pred_scores, "auc_score_binary")
    n, c = s.shape
    if n == 0 or c == 0:
        return 0, 0, 0, 0, 0
    lib = N.lib()
    nb = lib.osi_auc_workspace(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=s.device)
    counts = torch.zeros(5, dtype=torch.int64, device=s.device)
    fn = lib.osi_auc_binary_f32 if s.dtype == torch.float32 else lib.osi_auc_binary_f64
    N.check(fn(N.ptr(s), N.ptr(y), n, c, int(unk_class), N.ptr(ws), nb, N.ptr(counts), N.stream_of(s)), "osi_auc_binary")
    return tuple(int(v) for v in counts.cpu())


def _auc_ovr_counts(target_labels, pred_scores):
    """The device's integers for the one-vs-rest case: per-class lists gt, eq, P and (labels outside 0..C-1, NaN rows, rows that do
    not sum to 1)."""
    y, s = _auc_inputs(target_labels, pred_scores, "auc_score_multiclass")
    n, c = s.shape
    if n == 0 or c == 0:
        raise ValueError("auc_score_multiclass needs at least one sample and one class")
    lib = N.lib()
    nb = lib.osi_auc_workspace(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=s.device)
    out = torch.zeros(3 * c + 3, dtype=torch.int64, device=s.device)
    fn = lib.osi_auc_ovr_f32 if s.dtype == torch.float32 else lib.osi_auc_ovr_f64
    N.check(fn(N.ptr(s), N.ptr(y), n, c, N.ptr(ws), nb, N.ptr(out[:c]), N.ptr(out[c:2 * c]), N.ptr(out[2 * c:3 * c]), N.ptr(out[3 * c:]),
               N.stream_of(s)), "osi_auc_ovr")
    host = [int(v) for v in out.cpu()]
    return host[:c], host[c:2 * c], host[2 * c:3 * c], tuple(host[3 * c:])


def auc_score_binary(target_labels, pred_scores, unk_class=-1):
    """Binary ROC-AUC of known samples (label != unk_class) against the rest on the maximum score over all columns (reference
    metrics.py:65-88; for the garbage loss the caller drops the background column first, as the reference's docstring says).

    Returns nan when only one side is present (sklearn 1.7 warns and returns nan; older versions raise); ValueError on NaN scores."""
    gt, eq, pos, neg, nan_rows = _auc_binary_counts(target_labels, pred_scores, unk_class)
    if nan_rows:
        raise ValueError("Input contains NaN.")
    return _mann_whitney(gt, eq, pos, neg)


def auc_score_multiclass(target_labels, pred_scores):
    """One-vs-rest ROC-AUC, unweighted mean over the classes in column order (reference metrics.py:91-106:
    roc_auc_score(..., multi_class="ovr")). Like sklearn it refuses with ValueError: NaN scores, rows that are not probabilities
    (fp64 row sum off 1 by more than 1e-8 + 1e-5), a label outside 0..C-1 or a class without a sample."""
    gt, eq, pos, (bad_label, nan_rows, bad_sum) = _auc_ovr_counts(target_labels, pred_scores)
    n = sum(pos) + bad_label                              # every row is a positive of one class or carries a label outside 0..C-1
    if nan_rows:
        raise ValueError("Input contains NaN.")
    if bad_sum:
        raise ValueError("Target scores need to be probabilities for multiclass roc_auc, i.e. they should sum up to 1.0 over classes")
    if bad_label or not all(pos):
        raise ValueError("Number of classes in y_true not equal to the number of columns in 'y_score'")
    a = [_mann_whitney(gt[k], eq[k], pos[k], n - pos[k]) for k in range(len(pos))]
    return float(np.mean(np.asarray(a, dtype=np.float64)))

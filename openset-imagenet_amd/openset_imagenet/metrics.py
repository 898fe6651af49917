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
  detection_metrics(gt, unknown, unk_label=-2, tpr=(0.95,), correct=None)                   this build's addition
        -> dict: AUROC, AUPR-in, AUPR-out and FPR at TPR of a rejection score (the `unknown` vector of the post-hoc detectors), from
           six rank counts per row made on the device (osi_det_ranks_* / osi_det_summary, csrc/detection.hip).
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


def _detection_inputs(gt, unknown, correct, what):
    """Labels (int64), the rejection score u[N] (fp32 / fp64 kept, anything else cast to fp64) and the optional `correct` flags
    (uint8) on the current device, under the conventions of _auc_inputs. Copies only: the caller's arrays are never written."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"openset_imagenet (MI355X build) has no CPU path: {what} needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    u = torch.as_tensor(unknown).detach()
    if u.dtype not in (torch.float32, torch.float64):
        u = u.double()
    if u.dim() != 1:
        raise ValueError("unknown must be a vector [N_samples]")
    u = u.to(dev).contiguous()
    y = gt.detach() if isinstance(gt, torch.Tensor) else torch.as_tensor(np.asarray(gt).astype(int))
    y = y.to(torch.int64).to(dev).contiguous()
    if y.dim() != 1 or y.numel() != u.numel():
        raise ValueError("gt and unknown disagree on the number of samples")
    c = None
    if correct is not None:
        c = (torch.as_tensor(correct).detach().to(dev) != 0).to(torch.uint8).contiguous()
        if c.dim() != 1 or c.numel() != u.numel():
            raise ValueError("correct and unknown disagree on the number of samples")
    return y, u, c


def _det_ranks_device(y, u, c, unk_label):
    """osi_det_ranks_* on device tensors: the int32 [6, N] ranks and the int64 counts {K, U, Kc, NaN rows}, both on the device, and the
    workspace (of osi_det_workspace(N) bytes) for the calls that follow."""
    if int(unk_label) >= 0:
        raise ValueError("unk_label must be negative: labels >= 0 are the known classes")
    n = u.numel()
    lib = N.lib()
    nb = lib.osi_det_workspace(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=u.device)
    ranks = torch.empty((6, n), dtype=torch.int32, device=u.device)
    counts = torch.empty(4, dtype=torch.int64, device=u.device)
    fn = lib.osi_det_ranks_f32 if u.dtype == torch.float32 else lib.osi_det_ranks_f64
    N.check(fn(N.ptr(u), N.ptr(y), N.ptr(c), n, int(unk_label), N.ptr(ws), nb, N.ptr(ranks), N.ptr(counts), N.stream_of(u)), "osi_det_ranks")
    return ranks, counts, ws


def _tpr_levels(tpr):
    levels = [float(t) for t in tpr]
    if not 1 <= len(levels) <= N.DET_MAX_Q or not all(0.0 < t <= 1.0 for t in levels):
        raise ValueError(f"tpr must hold 1 to {N.DET_MAX_Q} levels in (0, 1]")
    return levels


def _detection_ranks(gt, unknown, unk_label=-2, tpr=(0.95,), correct=None):
    """The device's integers behind detection_metrics: a dict with `ranks` (numpy int32 [6, N]: kn_lt, kn_le, unk_lt, unk_le, cor_lt,
    cor_le), `counts` = (K, U, Kc, NaN rows), `gt_pairs`, `eq_pairs`, `fpr_count` (one per tpr level) as Python ints and the two fp64
    sums `ap_in_sum`, `ap_out_sum` (definitions: include/osi.h, ABI 28)."""
    levels = _tpr_levels(tpr)
    y, u, c = _detection_inputs(gt, unknown, correct, "detection_metrics")
    n = u.numel()
    if n == 0:
        return dict(ranks=np.zeros((6, 0), dtype=np.int32), counts=(0, 0, 0, 0), gt_pairs=0, eq_pairs=0, fpr_count=[0] * len(levels),
                    ap_in_sum=0.0, ap_out_sum=0.0)
    ranks, counts, ws = _det_ranks_device(y, u, c, unk_label)
    q = torch.tensor(levels, dtype=torch.float64, device=u.device)
    out = torch.empty(6 + len(levels) + 2, dtype=torch.int64, device=u.device)    # counts4, ints[2 + Q], then the two sums as fp64 bits
    out[:4] = counts
    ints, sums = out[4:6 + len(levels)], out[6 + len(levels):]
    N.check(N.lib().osi_det_summary(N.ptr(ranks), N.ptr(y), n, int(unk_label), N.ptr(q), len(levels), N.ptr(ws), ws.numel(), N.ptr(ints),
                                    N.ptr(sums), N.stream_of(u)), "osi_det_summary")
    host = out.cpu()
    vals = host[:-2].tolist()
    ap_in, ap_out = host[-2:].view(torch.float64).tolist()
    return dict(ranks=ranks.cpu().numpy(), counts=tuple(vals[:4]), gt_pairs=vals[4], eq_pairs=vals[5], fpr_count=vals[6:],
                ap_in_sum=ap_in, ap_out_sum=ap_out)


def detection_metrics(gt, unknown, unk_label=-2, tpr=(0.95,), correct=None):
    """The figures the out-of-distribution literature reports for a rejection score `unknown` [N] (higher = more unknown; the `unknown`
    vector every detector of this package writes), known rows (gt >= 0) against the rows labelled `unk_label`; rows of any other
    negative label take no part. A dict of plain Python values:

      auroc        area under the ROC curve, the Mann-Whitney quotient of exact pair counts (one division)
      aupr_in      average precision with the known rows as the positive class (score -unknown)
      aupr_out     average precision with the unknown rows as the positive class (score unknown)
      fpr_at_tpr   per level of `tpr`: the share of unknown rows accepted at the first threshold that accepts that share of known rows
                   (sklearn's fpr[argmax(tpr >= level)] of roc_curve with known as the positive class)
      known, unknown   the sizes of the two sides

    Everything is counted on the device (csrc/detection.hip; definitions in include/osi.h, ABI 28) and agrees with sklearn's
    roc_auc_score, average_precision_score and roc_curve(drop_intermediate=False) up to fp64 rounding. Inputs as _auc_inputs takes
    them: numpy arrays or torch tensors, host or device, fp32 / fp64 kept, never written. `correct` only adds to the raw counts
    (_detection_ranks). ValueError("Input contains NaN.") when a value is NaN; nan figures when a side is empty."""
    r = _detection_ranks(gt, unknown, unk_label=unk_label, tpr=tpr, correct=correct)
    k, u, _, nan_rows = r["counts"]
    if nan_rows:
        raise ValueError("Input contains NaN.")
    both = k > 0 and u > 0
    nan = float("nan")
    return dict(auroc=_mann_whitney(r["gt_pairs"], r["eq_pairs"], k, u),
                aupr_in=r["ap_in_sum"] / k if both else nan,
                aupr_out=r["ap_out_sum"] / u if both else nan,
                fpr_at_tpr=[f / u if both else nan for f in r["fpr_count"]],
                known=k, unknown=u)

"""Numpy restatement of the detection metrics and the OSCR curve by rejection score (include/osi.h, ABI 28; csrc/detection.hip;
metrics.detection_metrics, util.oscr_by_rejection). Exact where the device is exact: ranks from np.sort + searchsorted, the pair counts
and FPR counts as Python ints, the two average-precision sums as fractions.Fraction rounded once, the curve from a plain loop over
the thresholds. A plain module, imported like the other oracles."""
from fractions import Fraction

import numpy as np


def populations(gt, u, unk_label, correct=None):
    """Boolean masks (known, unk, correct) and the number of NaN rows. A NaN row belongs to no population."""
    gt, u = np.asarray(gt).astype(np.int64), np.asarray(u)
    assert unk_label < 0
    nan = np.isnan(u)
    kn = (gt >= 0) & ~nan
    un = (gt == unk_label) & ~nan
    co = kn & (np.asarray(correct) != 0) if correct is not None else np.zeros(len(u), dtype=bool)
    return kn, un, co, int(nan.sum())


def ranks(gt, u, unk_label, correct=None):
    """int32 [6, N]: kn_lt, kn_le, unk_lt, unk_le, cor_lt, cor_le (zeros for a NaN row), and counts = (K, U, Kc, NaN rows)."""
    u = np.asarray(u)
    kn, un, co, nan_rows = populations(gt, u, unk_label, correct)
    out = np.zeros((6, len(u)), dtype=np.int32)
    live = ~np.isnan(u)
    for r, pop in enumerate((kn, un, co)):
        srt = np.sort(u[pop])
        out[2 * r, live] = np.searchsorted(srt, u[live], side="left")
        out[2 * r + 1, live] = np.searchsorted(srt, u[live], side="right")
    return out, (int(kn.sum()), int(un.sum()), int(co.sum()), nan_rows)


def summary(gt, u, unk_label, tpr=(0.95,), correct=None):
    """What metrics._detection_ranks returns, with the sums exact: ap_in_sum / ap_out_sum are Fractions."""
    rk, counts = ranks(gt, u, unk_label, correct)
    kn, un, _, _ = populations(gt, u, unk_label, correct)
    K, U = counts[:2]
    kn_lt, kn_le, unk_lt, unk_le = (rk[r].astype(np.int64) for r in range(4))
    gt_pairs = int(kn_lt[un].sum())
    eq_pairs = int((kn_le[un] - kn_lt[un]).sum())
    fpr_count = []
    for q in tpr:
        hit = [int(unk_le[i]) for i in np.flatnonzero(kn) if int(kn_le[i]) / K >= q]       # int / int: the fp64 quotient of both
        fpr_count.append(min(hit) if hit else U)
    ap_in = sum((Fraction(int(kn_le[i]), int(kn_le[i] + unk_le[i])) for i in np.flatnonzero(kn)), Fraction(0))
    ap_out = sum((Fraction(int(U - unk_lt[i]), int((U - unk_lt[i]) + (K - kn_lt[i]))) for i in np.flatnonzero(un)), Fraction(0))
    return dict(ranks=rk, counts=counts, gt_pairs=gt_pairs, eq_pairs=eq_pairs, fpr_count=fpr_count, ap_in_sum=ap_in, ap_out_sum=ap_out)


def metrics(gt, u, unk_label=-2, tpr=(0.95,)):
    """What metrics.detection_metrics returns, every value rounded once from its exact quotient."""
    s = summary(gt, u, unk_label, tpr)
    K, U, _, nan_rows = s["counts"]
    if nan_rows:
        raise ValueError("Input contains NaN.")
    nan = float("nan")
    both = K > 0 and U > 0
    return dict(auroc=(2 * s["gt_pairs"] + s["eq_pairs"]) / (2 * K * U) if both else nan,
                aupr_in=float(s["ap_in_sum"] / K) if both else nan,
                aupr_out=float(s["ap_out_sum"] / U) if both else nan,
                fpr_at_tpr=[f / U if both else nan for f in s["fpr_count"]],
                known=K, unknown=U)


def curve_counts(gt, u, unk_label, correct):
    """(taus, ccr_count, fpr_count, (D, K, U)): the D distinct values of the known rows in descending order and, for each value t,
    #{correct: u < t} and #{unk: u < t}. The curve is the first D - 1 entries."""
    u = np.asarray(u)
    kn, un, co, _ = populations(gt, u, unk_label, correct)
    taus = np.unique(u[kn])[::-1]                       # -0 and +0 are one value
    ccr, fpr = [], []
    for t in taus:
        ccr.append(int(np.sum(co & (u < t))))
        fpr.append(int(np.sum(un & (u < t))))
    return taus, np.asarray(ccr, dtype=np.int64), np.asarray(fpr, dtype=np.int64), (len(taus), int(kn.sum()), int(un.sum()))


def first_max_correct(gt, scores):
    """Rows whose first maximum is their label (np.argmax keeps the first); a row holding a NaN is not correct."""
    gt, s = np.asarray(gt).astype(np.int64), np.asarray(scores)
    return ((s.argmax(1) == gt) & ~np.isnan(s).any(1)).astype(np.uint8)


def oscr_by_rejection(gt, scores, u, unk_label=-1):
    """(ccr, fpr) as util.oscr_by_rejection returns them."""
    _, ccr, fpr, (d, K, U) = curve_counts(gt, u, unk_label, first_max_correct(gt, scores))
    pts = max(0, d - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ccr[:pts] / np.int64(K), fpr[:pts] / np.int64(U)


def load_cases(golden_dir):
    """tests/golden/detection_reference.npz as a list of dicts: name, gt, u, unk, tpr, auroc, aupr_in, aupr_out, fpr_at_tpr, refused."""
    import os
    G = np.load(os.path.join(golden_dir, "detection_reference.npz"))
    return [dict(name=str(n), gt=G[f"{n}.gt"], u=G[f"{n}.u"], unk=int(G[f"{n}.unk"]), tpr=tuple(G[f"{n}.tpr"].tolist()),
                 auroc=float(G[f"{n}.auroc"]), aupr_in=float(G[f"{n}.aupr_in"]), aupr_out=float(G[f"{n}.aupr_out"]),
                 fpr_at_tpr=G[f"{n}.fpr_at_tpr"].tolist(), refused=bool(G[f"{n}.refused"])) for n in G["names"]]

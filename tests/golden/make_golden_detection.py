"""Generates tests/golden/detection_reference.npz — DEV CONTAINER ONLY (needs sklearn; never runs on the GPU box).

Expected values of metrics.detection_metrics from sklearn.metrics on the rows of the two sides (known: gt >= 0, unknown: gt == unk;
rows of another negative label are dropped before sklearn sees them), with known as the positive class y and -u as its score:

    auroc       roc_auc_score(y, -u)
    aupr_in     average_precision_score(y, -u)
    aupr_out    average_precision_score(1 - y, u)
    fpr_at_tpr  fpr[argmax(tpr >= level)] of roc_curve(y, -u, drop_intermediate=False)

Two rules of this file, not of sklearn. (1) sklearn refuses infinite scores; all four figures depend on the order of the values only,
so a case holding +-Inf hands sklearn the dense ranks of u instead of u (`ranked` = 1 in the fixture). (2) With one side empty sklearn
warns and returns a mixture of nan and 0; the fixture stores nan throughout, which is what detection_metrics returns. A NaN score is
refused by sklearn with ValueError (`refused` = 1), as by detection_metrics.

Layout: `names` lists the cases; per case `<name>.gt` (int64), `<name>.u` (fp32 or fp64), `<name>.unk`, `<name>.tpr` (levels),
`<name>.auroc`, `<name>.aupr_in`, `<name>.aupr_out`, `<name>.fpr_at_tpr` (one per level), `<name>.refused`, `<name>.ranked`.
"""
import os
import warnings

import numpy as np
from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve

HERE = os.path.dirname(os.path.abspath(__file__))


def labels(rng, N, p_unk, p_other=0.0, unk=-2):
    gt = rng.integers(0, 10, size=N)
    r = rng.random(N)
    gt[r < p_unk] = unk
    gt[(r >= p_unk) & (r < p_unk + p_other)] = -3 - unk        # the other negative label
    return gt.astype(np.int64)


def separated(rng, gt, dtype, quant=None, shift=1.0):
    """Unknown rows score higher on average; `quant` cuts the values to multiples of 1 / quant (heavy ties)."""
    u = rng.normal(size=len(gt)) + shift * (gt < 0)
    if quant:
        u = np.round(u * quant) / quant
    return u.astype(dtype)


def cases():
    rng = np.random.default_rng(2028)
    out = []

    def add(name, gt, u, unk=-2, tpr=(0.95,)):
        out.append(dict(name=name, gt=gt, u=u, unk=unk, tpr=np.asarray(tpr, dtype=np.float64)))

    gt = labels(rng, 257, 0.4); add("mixed_f32", gt, separated(rng, gt, np.float32))
    gt = labels(rng, 300, 0.35); add("ties_f32", gt, separated(rng, gt, np.float32, quant=4), tpr=(0.5, 0.9, 0.95, 1.0))
    gt = labels(rng, 150, 0.5); add("ties_f64", gt, separated(rng, gt, np.float64, quant=2), tpr=(0.95, 0.99))
    gt = labels(rng, 513, 0.3); add("mixed_f64", gt, separated(rng, gt, np.float64))
    gt = labels(rng, 64, 0.5); add("all_tied", gt, np.full(64, 0.25, dtype=np.float32), tpr=(0.1, 0.95))
    gt = labels(rng, 64, 0.0); add("only_known", gt, separated(rng, gt, np.float32))
    gt = labels(rng, 64, 1.1); add("only_unknown", gt, separated(rng, gt, np.float32))
    add("one_row", np.array([3], dtype=np.int64), np.array([0.5], dtype=np.float32))
    add("two_rows", np.array([2, -2], dtype=np.int64), np.array([0.5, 0.75], dtype=np.float32), tpr=(0.95, 1.0))
    gt = labels(rng, 200, 0.4)
    u = separated(rng, gt, np.float32, quant=2); u[::9] = np.inf; u[4::11] = -np.inf
    add("infinities", gt, u, tpr=(0.5, 0.95))
    gt = labels(rng, 180, 0.25, p_other=0.2); add("minus1_beside_minus2", gt, separated(rng, gt, np.float32, quant=8))
    gt = labels(rng, 180, 0.25, p_other=0.2, unk=-1); add("unk_minus1", gt, separated(rng, gt, np.float32, quant=8), unk=-1)
    gt = labels(rng, 120, 0.4); u = separated(rng, gt, np.float32); u[57] = np.nan
    add("nan_refused", gt, u)
    gt = labels(rng, 240, 0.45); add("inverted", gt, separated(rng, gt, np.float64, quant=16, shift=-1.5), tpr=(0.8, 0.95))
    gt = labels(rng, 400, 0.5); u = separated(rng, gt, np.float32, quant=1); u[u == 0] = np.where(rng.random((u == 0).sum()) < 0.5, -0.0, 0.0)
    add("signed_zeros", gt, u.astype(np.float32))
    gt = labels(rng, 2000, 0.37); add("large", gt, separated(rng, gt, np.float32, quant=64), tpr=(0.9, 0.95, 0.99))
    return out


def reference(gt, u, unk, tpr):
    """(auroc, aupr_in, aupr_out, fpr_at_tpr, refused, ranked) under the rules of the module docstring."""
    nan = float("nan")
    sel = (gt >= 0) | (gt == unk)
    y, s = (gt[sel] >= 0).astype(np.int64), u[sel].astype(np.float64)
    if np.isnan(s).any():
        try:
            roc_auc_score(y, -s)
        except ValueError as e:
            print(f"    ValueError: {str(e)[:60]}")
            return nan, nan, nan, [nan] * len(tpr), 1, 0
        raise AssertionError("sklearn accepted a NaN score")
    if y.sum() == 0 or y.sum() == len(y):
        return nan, nan, nan, [nan] * len(tpr), 0, 0
    ranked = int(np.isinf(s).any())
    if ranked:
        s = np.searchsorted(np.unique(s), s).astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fpr, tp, _ = roc_curve(y, -s, drop_intermediate=False)
        return (float(roc_auc_score(y, -s)), float(average_precision_score(y, -s)), float(average_precision_score(1 - y, s)),
                [float(fpr[np.argmax(tp >= q)]) for q in tpr], 0, ranked)


def main():
    out, names = {}, []
    for c in cases():
        n = c["name"]
        auroc, ap_in, ap_out, fprs, refused, ranked = reference(c["gt"], c["u"], c["unk"], c["tpr"])
        out[f"{n}.gt"], out[f"{n}.u"], out[f"{n}.unk"], out[f"{n}.tpr"] = c["gt"], c["u"], np.int64(c["unk"]), c["tpr"]
        out[f"{n}.auroc"], out[f"{n}.aupr_in"], out[f"{n}.aupr_out"] = np.float64(auroc), np.float64(ap_in), np.float64(ap_out)
        out[f"{n}.fpr_at_tpr"], out[f"{n}.refused"], out[f"{n}.ranked"] = np.asarray(fprs, dtype=np.float64), np.int64(refused), np.int64(ranked)
        names.append(n)
        print(f"{n:22s} N={len(c['gt']):5d} {str(c['u'].dtype):8s} unk={c['unk']} refused={refused} ranked={ranked} auroc={auroc!r} "
              f"aupr_in={ap_in!r} aupr_out={ap_out!r} fpr_at_tpr={fprs}")
    out["names"] = np.array(names)
    path = os.path.join(HERE, "detection_reference.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

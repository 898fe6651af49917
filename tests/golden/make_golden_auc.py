"""Generates tests/golden/auc_reference.npz — DEV CONTAINER ONLY (needs /root/reference and sklearn; never runs on the GPU box).

Executes the reference's OWN `auc_score_binary` / `auc_score_multiclass` (/root/reference/openset_imagenet/metrics.py:65-106, thin
wrappers around sklearn.metrics.roc_auc_score). The module needs numpy, sklearn.metrics and torch only, so it is loaded by file path
as it is. `auc_score_binary` overwrites the labels it is given with +-1, so both functions get COPIES. Only arrays go into the
fixture: inputs, expected values and, for the inputs the reference refuses with ValueError, a flag.

Layout: `names` lists the cases; per case `<name>.kind` ("binary" / "multiclass"), `<name>.gt`, `<name>.scores_id` (score matrices
are pooled under `scores.<id>`: a binary and a multiclass case may read the same matrix), `<name>.unk` (binary), `<name>.auc`
(float64, nan where the reference returns nan or refuses) and `<name>.refused` (1 = ValueError).
"""
import importlib.util
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_FILE = "/root/reference/openset_imagenet/metrics.py"


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_metrics", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def softmax_scores(rng, N, C, dtype, quant=None):
    z = rng.normal(size=(N, C)) * 2
    s = np.exp(z - z.max(1, keepdims=True)); s /= s.sum(1, keepdims=True)
    if quant:
        s = np.round(s * quant) / quant
    return s.astype(dtype)


def labels_every_class(rng, N, C):
    gt = np.concatenate([np.arange(C), rng.integers(0, C, size=N - C)])
    rng.shuffle(gt)
    return gt.astype(np.int64)


def cases():
    rng = np.random.default_rng(2025)
    pool, out = {}, []

    def binary(name, sid, unk=-1, p_neg=0.4, p_other=0.0):
        N, C = pool[sid].shape
        gt = rng.integers(0, C, size=N)
        r = rng.random(N)
        gt[r < p_neg] = -1
        gt[(r >= p_neg) & (r < p_neg + p_other)] = -2
        out.append(dict(name=name, kind="binary", gt=gt.astype(np.int64), sid=sid, unk=unk))

    def multiclass(name, sid, gt=None):
        N, C = pool[sid].shape
        out.append(dict(name=name, kind="multiclass", gt=labels_every_class(rng, N, C) if gt is None else gt.astype(np.int64), sid=sid, unk=0))

    def tied_rows(s):                       # every fifth row repeats the row three above it: ties in every column, row sums intact
        s, idx = s.copy(), np.arange(5, len(s), 5)
        s[idx] = s[idx - 3]
        return s

    pool["s257x30"] = tied_rows(softmax_scores(rng, 257, 30, np.float32))
    pool["q300x8"] = softmax_scores(rng, 300, 8, np.float32, quant=16)
    pool["q150x5_f64"] = softmax_scores(rng, 150, 5, np.float64, quant=8)
    pool["s180x10"] = softmax_scores(rng, 180, 10, np.float32)
    pool["s64x6"] = softmax_scores(rng, 64, 6, np.float32)
    pool["s1x4"] = softmax_scores(rng, 1, 4, np.float32)
    pool["s2x4"] = softmax_scores(rng, 2, 4, np.float32)
    pool["const50x7"] = np.full((50, 7), 1.0 / 7, dtype=np.float32)
    pool["s2000x30"] = tied_rows(softmax_scores(rng, 2000, 30, np.float32))
    pool["s300x8"] = tied_rows(softmax_scores(rng, 300, 8, np.float32))
    pool["s512x5_f64"] = tied_rows(softmax_scores(rng, 512, 5, np.float64))
    pool["quarter64x6"] = softmax_scores(rng, 64, 6, np.float32, quant=4)      # rows no longer sum to 1

    binary("bin_mixed", "s257x30")
    binary("bin_ties", "q300x8", p_neg=0.35)
    binary("bin_ties_f64", "q150x5_f64", p_neg=0.5)
    binary("bin_unk_minus2", "s180x10", unk=-2, p_neg=0.2, p_other=0.25)
    binary("bin_only_positives", "s64x6", p_neg=0.0)
    binary("bin_only_negatives", "s64x6", p_neg=1.1)
    binary("bin_one_row", "s1x4", p_neg=0.0)
    binary("bin_two_rows", "s2x4", p_neg=0.0)
    out[-1]["gt"] = np.array([2, -1], dtype=np.int64)
    binary("bin_all_equal", "const50x7", p_neg=0.5)
    binary("bin_large", "s2000x30", p_neg=0.37)

    multiclass("mc_257x30", "s257x30")
    multiclass("mc_300x8", "s300x8")
    multiclass("mc_512x5_f64", "s512x5_f64")
    multiclass("mc_large", "s2000x30")
    lone = rng.integers(0, 5, size=64); lone[17] = 5
    multiclass("mc_class_with_one_sample", "s64x6", gt=lone)
    neg = labels_every_class(rng, 64, 6); neg[3] = -1
    multiclass("mc_refuse_negative_label", "s64x6", gt=neg)
    multiclass("mc_refuse_missing_class", "s64x6", gt=rng.integers(0, 5, size=64))
    multiclass("mc_refuse_not_probabilities", "quarter64x6")
    return pool, out


def main():
    ref = load_reference()
    pool, cs = cases()
    out = {f"scores.{k}": v for k, v in pool.items()}
    for c in cs:
        name, gt, s = c["name"], c["gt"], pool[c["sid"]]
        refused, value = 0, float("nan")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                if c["kind"] == "binary":
                    value = float(ref.auc_score_binary(gt.copy(), s.copy(), unk_class=c["unk"]))
                else:
                    value = float(ref.auc_score_multiclass(gt.copy(), s.copy()))
            except ValueError as e:
                refused = 1
                print(f"    {name}: ValueError: {str(e)[:90]}")
        out[f"{name}.kind"], out[f"{name}.gt"], out[f"{name}.scores_id"] = np.array(c["kind"]), gt, np.array(c["sid"])
        out[f"{name}.unk"], out[f"{name}.auc"], out[f"{name}.refused"] = np.int64(c["unk"]), np.float64(value), np.int64(refused)
        print(f"{name:30s} N={len(gt):5d} C={s.shape[1]:3d} {str(s.dtype):8s} refused={refused} auc={value!r}")
    out["names"] = np.array([c["name"] for c in cs])
    path = os.path.join(HERE, "auc_reference.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

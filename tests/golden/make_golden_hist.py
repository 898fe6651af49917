"""Generates tests/golden/hist_reference.npz — DEV CONTAINER ONLY (needs a checkout of the reference, named by the environment
variable OSI_REFERENCE_DIR, and whatever its util.py imports; never runs on the GPU box).

Executes the reference's OWN `get_histogram` (openset_imagenet/util.py:202-228 of the reference), loaded by file path as it is. Only
arrays go into the fixture: inputs, the four outputs and, for the inputs the reference refuses, a flag.

Layout: `names` lists the cases; per case `<name>.gt`, `<name>.scores_id` / `<name>.features_id` (matrices are pooled under
`scores.<id>` / `features.<id>`), the arguments `<name>.unk`, `<name>.metric` ("score" / "norm"), `<name>.bins`, `<name>.drop_bg`,
`<name>.log_space`, `<name>.limits` (2 floats), the outputs `<name>.kn_hist`, `<name>.kn_edges`, `<name>.unk_hist`,
`<name>.unk_edges` (empty arrays when refused) and `<name>.refused` (0 = answered, 1 = IndexError, 2 = ValueError).

Norm cases use integer-valued features in -3 .. 3: sums of squares are then exact in every order and precision, and the square
root in double rounded once to the features' type is the correctly rounded root, so the reference's norms (np.linalg.norm in the
features' dtype) and the device's are the same bits.
"""
import importlib.util
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference():
    path = os.path.join(os.environ["OSI_REFERENCE_DIR"], "openset_imagenet", "util.py")
    spec = importlib.util.spec_from_file_location("reference_util", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def softmax_scores(rng, N, C, dtype, quant=None):
    z = rng.normal(size=(N, C)) * 2
    s = np.exp(z - z.max(1, keepdims=True)); s /= s.sum(1, keepdims=True)
    if quant:
        s = np.round(s * quant) / quant
    return s.astype(dtype)


def labels(rng, N, classes, p_neg=0.25, p_unk=0.25):
    gt = rng.integers(0, classes, size=N)
    r = rng.random(N)
    gt[r < p_neg] = -1
    gt[(r >= p_neg) & (r < p_neg + p_unk)] = -2
    return gt.astype(np.int64)


def cases():
    rng = np.random.default_rng(2026)
    scores, feats, out = {}, {}, []
    scores["s600x12"] = softmax_scores(rng, 600, 12, np.float32)
    scores["s300x7_f64"] = softmax_scores(rng, 300, 7, np.float64)
    q = softmax_scores(rng, 400, 8, np.float32, quant=64)
    q[0] = 0; q[0, 3] = 1.0                                    # a known row with target score 1 and one with 0: the range is [0, 1]
    q[1] = 0; q[1, 5] = 1.0
    scores["q400x8"] = q
    scores["const50x7"] = np.full((50, 7), 1.0 / 7, dtype=np.float32)
    bad = scores["s600x12"][:200].copy()
    scores["nan200x12"] = bad
    feats["f600x16"] = rng.integers(-3, 4, size=(600, 16)).astype(np.float32)
    feats["f300x16_f64"] = rng.integers(-3, 4, size=(300, 16)).astype(np.float64)

    def feat_for(sid):
        N, dt = scores[sid].shape[0], scores[sid].dtype
        return "f300x16_f64" if dt == np.float64 else "f600x16"

    def add(name, sid, gt, unk=-1, metric="score", bins=100, drop_bg=False, log_space=False, limits=(1, 1e2)):
        out.append(dict(name=name, sid=sid, fid=feat_for(sid), gt=gt, unk=unk, metric=metric, bins=bins, drop_bg=drop_bg,
                        log_space=log_space, limits=limits))

    add("f32_bins100_neg", "s600x12", labels(rng, 600, 12), unk=-1, bins=100)
    add("f32_bins30_unk", "s600x12", labels(rng, 600, 12), unk=-2, bins=30)
    add("f32_bins1_neg", "s600x12", labels(rng, 600, 12), unk=-1, bins=1)
    add("f64_bins30_neg", "s300x7_f64", labels(rng, 300, 7), unk=-1, bins=30)
    add("f64_bins100_unk", "s300x7_f64", labels(rng, 300, 7), unk=-2, bins=100)
    add("f64_bins1_unk", "s300x7_f64", labels(rng, 300, 7), unk=-2, bins=1)
    add("gt_as_float32", "s600x12", labels(rng, 600, 12).astype(np.float32), unk=-2, bins=30)
    add("no_unknown_rows", "s600x12", labels(rng, 600, 12, p_unk=0.0), unk=-2, bins=30)
    add("no_known_rows", "s600x12", labels(rng, 600, 12, p_neg=0.5, p_unk=0.6), unk=-1, bins=30)
    one = labels(rng, 300, 7, p_unk=0.0); one[17] = -2
    add("one_unknown_row", "s300x7_f64", one, unk=-2, bins=30)
    add("equal_values", "const50x7", labels(rng, 50, 7), unk=-1, bins=30)
    gq = labels(rng, 400, 8); gq[0] = 3; gq[1] = 2; gq[2] = -1; gq[3] = -2
    add("quantised_bins32", "q400x8", gq, unk=-1, bins=32)
    add("quantised_bins100", "q400x8", gq, unk=-2, bins=100)
    add("drop_bg_ok", "s600x12", labels(rng, 600, 11), unk=-1, bins=30, drop_bg=True)
    gb = labels(rng, 600, 11); gb[np.flatnonzero(gb >= 0)[5]] = 11
    add("drop_bg_label_is_bg", "s600x12", gb, unk=-1, bins=30, drop_bg=True)
    gn = labels(rng, 200, 12); gn[40] = 6; bad[40, 6] = np.nan
    add("nan_score", "nan200x12", gn, unk=-1, bins=30)
    add("log_default_limits", "s600x12", labels(rng, 600, 12), unk=-1, bins=30, log_space=True)
    add("log_limits_0.1_10", "s300x7_f64", labels(rng, 300, 7), unk=-2, bins=100, log_space=True, limits=(0.1, 10))
    add("norm_f32_bins30", "s600x12", labels(rng, 600, 12), unk=-2, metric="norm", bins=30)
    add("norm_f64_bins100", "s300x7_f64", labels(rng, 300, 7), unk=-1, metric="norm", bins=100)
    add("norm_log_default_limits", "s300x7_f64", labels(rng, 300, 7), unk=-2, metric="norm", bins=30, log_space=True)
    add("norm_log_limits_0.1_10","s600x12", labels(rng, 600, 12), unk=-1, metric="norm", bins=30, log_space=True, limits=(0.1, 10))
    return scores, feats, out


def main():
    ref = load_reference()
    scores, feats, cs = cases()
    out = {f"scores.{k}": v for k, v in scores.items()}
    out.update({f"features.{k}": v for k, v in feats.items()})
    none = np.zeros(0)
    for c in cs:
        name, s = c["name"], scores[c["sid"]]
        f = feats[c["fid"]][:len(s)]
        refused, res = 0, (none, none, none, none)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                res = ref.get_histogram(dict(scores=s.copy(), gt=c["gt"].copy(), features=f.copy()), unk_label=c["unk"],
                                        metric=c["metric"], bins=c["bins"], drop_bg=c["drop_bg"], log_space=c["log_space"],
                                        geomspace_limits=c["limits"])
            except IndexError as e:
                refused = 1
                print(f"    {name}: IndexError: {str(e)[:90]}")
            except ValueError as e:
                refused = 2
                print(f"    {name}: ValueError: {str(e)[:90]}")
        out[f"{name}.gt"], out[f"{name}.scores_id"], out[f"{name}.features_id"] = c["gt"], np.array(c["sid"]), np.array(c["fid"])
        out[f"{name}.unk"], out[f"{name}.metric"], out[f"{name}.bins"] = np.int64(c["unk"]), np.array(c["metric"]), np.int64(c["bins"])
        out[f"{name}.drop_bg"], out[f"{name}.log_space"] = np.int64(c["drop_bg"]), np.int64(c["log_space"])
        out[f"{name}.limits"], out[f"{name}.refused"] = np.asarray(c["limits"], dtype=np.float64), np.int64(refused)
        for key, v in zip(("kn_hist", "kn_edges", "unk_hist", "unk_edges"), res):
            out[f"{name}.{key}"] = np.asarray(v)
        print(f"{name:26s} N={len(s):4d} C={s.shape[1]:3d} {str(s.dtype):8s} refused={refused} "
              f"kn={int(np.sum(res[0]))} ({np.asarray(res[1]).dtype}) unk={int(np.sum(res[2]))} ({np.asarray(res[3]).dtype})")
    out["names"] = np.array([c["name"] for c in cs])
    path = os.path.join(HERE, "hist_reference.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

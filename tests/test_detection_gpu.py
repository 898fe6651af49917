"""GPU parity of the detection metrics and the OSCR curve by rejection score (metrics.detection_metrics, util.oscr_by_rejection,
csrc/detection.hip; include/osi.h, ABI 28): sklearn's values (tests/golden/detection_reference.npz) within 1e-12, and the integers of
the numpy oracle (tests/detection_oracle.py) exactly: ranks, pair counts, FPR counts, curve counts. The two fp64 sums are held to
the error bound of their fixed-order tree."""
import struct

import numpy as np
import pytest
import torch

import detection_oracle as O
import gpu_harness as H

pytestmark = pytest.mark.gpu

# One fp64 division per term, then at most 19 additions on the way to the result for N <= 65536 (butterfly 6, waves 3, one strided
# step, butterfly 6, waves 3); every term is positive, so the relative error of a sum is at most 20 roundings, plus one for the oracle.
SUM_RTOL = 21 * 2.0 ** -53


def same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def quantised(rng, gt, dtype, shift=0.75):
    """Multiples of 1 / 16 in a narrow range (ties on every side), the unknown rows higher on average."""
    return (np.round((rng.random(len(gt)) * 3 + shift * (np.asarray(gt) < 0)) * 16) / 16).astype(dtype)


def abi_run(dev, gt, u, unk, correct=None, tpr=(0.95,)):
    """The three C-ABI calls on guard-banded outputs, each with a workspace of its own poisoned with 0xFF. Returns a dict of numpy
    arrays after checking every guard band."""
    from openset_imagenet import _native as NL
    lib = NL.lib()
    n = len(u)
    f32 = u.dtype == np.float32
    g, x, c, q = H.on(dev, np.asarray(gt, dtype=np.int64), u, None if correct is None else np.asarray(correct, dtype=np.uint8),
                      np.asarray(tpr, dtype=np.float64))
    nb = lib.osi_det_workspace(n)
    assert nb >= 16 * n
    outs = dict(ranks=H.Out((6, n), torch.int32, dev), counts=H.Out((4,), torch.int64, dev), ints=H.Out((2 + len(tpr),), torch.int64, dev),
                sums=H.Out((2,), torch.float64, dev), taus=H.Out((n,), torch.float32 if f32 else torch.float64, dev),
                ccr=H.Out((n,), torch.int64, dev), fpr=H.Out((n,), torch.int64, dev), totals=H.Out((3,), torch.int64, dev))
    H.call(lib.osi_det_ranks_f32 if f32 else lib.osi_det_ranks_f64, x, g, c, n, unk, H.poisoned(nb, dev), nb, outs["ranks"], outs["counts"])
    H.call(lib.osi_det_summary, outs["ranks"], g, n, unk, q, len(tpr), H.poisoned(nb, dev), nb, outs["ints"], outs["sums"])
    H.call(lib.osi_det_curve_f32 if f32 else lib.osi_det_curve_f64, x, g, outs["ranks"], n, unk, H.poisoned(nb, dev), nb, outs["taus"],
           outs["ccr"], outs["fpr"], outs["totals"])
    for name, o in outs.items():
        assert o.check(), f"{name}: guard band overwritten"
    assert np.array_equal(x.cpu().numpy(), u, equal_nan=True) and np.array_equal(g.cpu().numpy(), gt)       # inputs unmodified
    return {k: o.np() for k, o in outs.items()}


def check_against_oracle(got, gt, u, unk, correct, tpr, what):
    want = O.summary(gt, u, unk, tpr, correct)
    for r, row in enumerate(("kn_lt", "kn_le", "unk_lt", "unk_le", "cor_lt", "cor_le")):
        assert np.array_equal(got["ranks"][r], want["ranks"][r]), (what, row)
    assert tuple(got["counts"].tolist()) == want["counts"], what
    assert got["ints"].tolist() == [want["gt_pairs"], want["eq_pairs"]] + want["fpr_count"], what
    for mine, exact in zip(got["sums"].tolist(), (want["ap_in_sum"], want["ap_out_sum"])):
        assert abs(mine - float(exact)) <= SUM_RTOL * float(exact), (what, mine, float(exact))
    taus, ccr, fpr, totals = O.curve_counts(gt, u, unk, correct if correct is not None else np.zeros(len(u), dtype=np.uint8))
    d = totals[0]
    assert tuple(got["totals"].tolist()) == totals, what
    assert np.array_equal(got["taus"][:d], taus) and np.array_equal(got["ccr"][:d], ccr) and np.array_equal(got["fpr"][:d], fpr), what
    assert not got["taus"][d:].any() and not got["ccr"][d:].any() and not got["fpr"][d:].any(), what        # zeroed past the curve
    return want


def test_fixture_cases_host_and_device_inputs(cuda, golden_dir):
    from openset_imagenet.metrics import _detection_ranks, detection_metrics
    worst = 0.0
    for c in O.load_cases(golden_dir):
        gt, u = c["gt"], c["u"]
        for where in ("host", "device"):
            y, x = (gt.copy(), u.copy()) if where == "host" else (torch.from_numpy(gt).to(cuda), torch.from_numpy(u).to(cuda))
            if c["refused"]:
                with pytest.raises(ValueError, match="Input contains NaN"):
                    detection_metrics(y, x, unk_label=c["unk"], tpr=c["tpr"])
            else:
                got = detection_metrics(y, x, unk_label=c["unk"], tpr=c["tpr"])
                assert all(type(got[k]) is float for k in ("auroc", "aupr_in", "aupr_out")) and type(got["known"]) is int
                pairs = [(got[k], c[k]) for k in ("auroc", "aupr_in", "aupr_out")] + list(zip(got["fpr_at_tpr"], c["fpr_at_tpr"]))
                assert len(got["fpr_at_tpr"]) == len(c["tpr"])
                for mine, ref in pairs:
                    if np.isnan(ref):
                        assert np.isnan(mine), (c["name"], where)
                    else:
                        worst = max(worst, abs(mine - ref))
                        assert abs(mine - ref) <= 1e-12, (c["name"], where, mine, ref)
                raw, want = _detection_ranks(y, x, unk_label=c["unk"], tpr=c["tpr"]), O.summary(gt, u, c["unk"], c["tpr"])
                assert np.array_equal(raw["ranks"], want["ranks"]) and raw["counts"] == want["counts"], (c["name"], where)
                assert (raw["gt_pairs"], raw["eq_pairs"], raw["fpr_count"]) == (want["gt_pairs"], want["eq_pairs"], want["fpr_count"])
                assert (got["known"], got["unknown"]) == want["counts"][:2]
            y2, x2 = (y, x) if where == "host" else (y.cpu().numpy(), x.cpu().numpy())
            assert H.same_bytes(y2, gt) and H.same_bytes(x2, u), (c["name"], where)
    print(f"largest |device - sklearn| over the fixture: {worst:.3e}")


def edge_cases():
    """(N, K, U, Kc): N around the 256-wide tiles, every population numbering 0, 1, 256 or 257 where it fits (from either end)."""
    out = []
    for N in (1, 2, 255, 256, 257, 513):
        sizes = sorted({p for k in (0, 1, 256, 257) for p in (k, N - k) if 0 <= p <= N})
        for K in sizes:
            c_sizes = sorted({s for s in (0, 1, 256, 257, K) if s <= K})
            for U in sorted({s for s in (0, 1, 256, 257, N - K) if s <= N - K}):
                out.append((N, K, U, c_sizes[len(out) % len(c_sizes)]))
    return out


EDGES = edge_cases()


def test_tile_edges(cuda):
    seen = {"K": set(), "U": set(), "Kc": set()}
    ties = 0
    rng = np.random.default_rng(28)
    for n, (N, K, U, Kc) in enumerate(EDGES):
        dtype = np.float64 if n % 2 else np.float32
        unk = -2 if n % 3 else -1
        gt = np.full(N, -3 - unk, dtype=np.int64)                      # the other negative label: no population
        order = rng.permutation(N)
        gt[order[:K]] = rng.integers(0, 5, size=K)
        gt[order[K:K + U]] = unk
        correct = np.zeros(N, dtype=np.uint8)
        correct[order[:Kc]] = 1
        correct[order[K:]] = rng.integers(0, 2, size=N - K)            # set on rows that are not known: must not count
        u = quantised(rng, gt, dtype)
        tpr = (0.5, 0.95, 1.0)
        runs = []

        def run():
            runs.append(abi_run(cuda, gt, u, unk, correct, tpr))
            return np.concatenate([v.ravel().astype(np.float64) for v in runs[-1].values()])

        assert H.twice(run).shape == (6 * N + 4 + 5 + 2 + 3 * N + 3,)
        got = runs[-1]
        want = check_against_oracle(got, gt, u, unk, correct, tpr, (N, K, U, Kc, dtype.__name__))
        assert want["counts"] == (K, U, Kc, 0)
        if N >= 255:
            assert len(np.unique(u)) < N                               # 1 / 16 steps over less than 4 units: ties
        ties += want["eq_pairs"]
        for key, v in (("K", K), ("U", U), ("Kc", Kc)):
            seen[key].add(v)
    assert ties > 0
    for key in seen:
        assert {0, 1, 256, 257} <= seen[key], (key, sorted(seen[key]))


def test_sums_have_the_same_bits_in_two_runs(cuda):
    """gpu_harness.twice compares as fp32; the fp64 sums and every integer are compared here byte for byte."""
    rng = np.random.default_rng(4)
    gt = rng.integers(0, 7, size=1500); gt[rng.random(1500) < 0.4] = -2
    u = quantised(rng, gt, np.float32)
    a, b = abi_run(cuda, gt, u, -2, None, (0.9,)), abi_run(cuda, gt, u, -2, None, (0.9,))
    for key in a:
        assert H.same_bytes(a[key], b[key]), key
    assert a["sums"][0] > 0 and a["counts"][2] == 0 and not a["ranks"][4:].any() and not a["ccr"].any()      # correct = NULL: empty


def test_counts_past_32_bits(cuda):
    from openset_imagenet.metrics import _detection_ranks, detection_metrics
    N = 140000
    u = torch.full((N,), 0.5, dtype=torch.float32, device=cuda)
    gt = torch.zeros(N, dtype=torch.int64, device=cuda)
    gt[::2] = -2
    raw = _detection_ranks(gt, u)
    assert (raw["gt_pairs"], raw["eq_pairs"], raw["counts"]) == (0, 4900000000, (70000, 70000, 0, 0))
    got = detection_metrics(gt, u)
    assert got["auroc"] == 0.5 and got["aupr_in"] == 0.5 and got["aupr_out"] == 0.5 and got["fpr_at_tpr"] == [1.0]


def test_auroc_has_the_bits_of_auc_score_binary(cuda):
    from openset_imagenet.metrics import auc_score_binary, detection_metrics
    rng = np.random.default_rng(16)
    for dtype, unk in ((np.float32, -2), (np.float64, -1)):
        gt = rng.integers(0, 9, size=900); r = rng.random(900); gt[r < 0.3] = -2; gt[r > 0.8] = -1
        u = quantised(rng, gt, dtype)
        sel = (gt >= 0) | (gt == unk)
        want = auc_score_binary(gt[sel], (-u[sel])[:, None], unk)
        got = detection_metrics(gt, u, unk_label=unk)["auroc"]
        assert 0.5 < got < 1.0 and same_bits(got, want), (dtype, got, want)


def test_oscr_by_rejection(cuda):
    from openset_imagenet.util import calculate_oscr, oscr_area, oscr_by_rejection
    rng = np.random.default_rng(12)
    N, C = 700, 6
    gt = rng.integers(0, C, size=N); r = rng.random(N); gt[r < 0.3] = -1; gt[r > 0.85] = -2
    for dtype in (np.float32, np.float64):
        # every known row classified correctly: with u = -max score the curve is calculate_oscr's, bit for bit
        s = (np.round(rng.random((N, C)) * 8) / 16).astype(dtype)
        kn = np.flatnonzero(gt >= 0)
        s[kn, gt[kn]] = (0.5625 + np.round(rng.random(len(kn)) * 7) / 16).astype(dtype)
        assert O.first_max_correct(gt, s)[kn].all()                    # checked on the CPU
        for unk in (-1, -2):
            for where in ("host", "device"):
                y, x = (gt, s) if where == "host" else (torch.from_numpy(gt).to(cuda), torch.from_numpy(s).to(cuda))
                ccr, fpr = oscr_by_rejection(y, x, -x.max(1) if where == "host" else -x.max(1).values, unk_label=unk)
                ref_ccr, ref_fpr = calculate_oscr(gt, s, unk_label=unk)
                assert len(ccr) > 5 and ccr.dtype == np.float64 and H.same_bytes(ccr, ref_ccr) and H.same_bytes(fpr, ref_fpr), (dtype, unk, where)
        # in general (wrong predictions, first-maximum ties, a rejector of its own): the oracle's integers
        s = (np.round(rng.random((N, C)) * 4) / 4).astype(dtype)
        u = quantised(rng, gt, dtype)
        assert 0 < O.first_max_correct(gt, s)[kn].sum() < len(kn)
        ccr, fpr = oscr_by_rejection(gt, s, u, unk_label=-2)
        want_ccr, want_fpr = O.oscr_by_rejection(gt, s, u, unk_label=-2)
        assert len(ccr) > 5 and H.same_bytes(ccr, want_ccr) and H.same_bytes(fpr, want_fpr)
        assert (np.diff(fpr) <= 0).all() and 0.0 < oscr_area(ccr, fpr) < 1.0
    with pytest.raises(ValueError, match="NaN"):
        oscr_by_rejection(gt, s, np.where(np.arange(N) == 5, np.nan, u), unk_label=-2)


def test_label_and_value_edge_rows(cuda):
    """NaN rows belong to no population and are counted; rows of the other negative label take no part, whichever of -1 / -2 is the
    unknown one; +-Inf rank as the extremes; -0 ties with +0."""
    from openset_imagenet.metrics import _detection_ranks, detection_metrics
    rng = np.random.default_rng(9)
    N = 600
    for dtype in (np.float32, np.float64):
        gt = rng.integers(0, 4, size=N); r = rng.random(N); gt[r < 0.3] = -1; gt[r > 0.7] = -2
        u = quantised(rng, gt, dtype) - 2                              # zeros occur
        u[u == 0] = np.where(rng.random(int((u == 0).sum())) < 0.5, -0.0, 0.0)
        assert (np.signbit(u) & (u == 0)).any() and (~np.signbit(u) & (u == 0)).any()
        u[rng.permutation(N)[:40]] = np.inf
        u[rng.permutation(N)[:40]] = -np.inf
        correct = rng.integers(0, 2, size=N).astype(np.uint8)
        for unk in (-1, -2):
            got = abi_run(cuda, gt, u, unk, correct, (0.95,))
            want = check_against_oracle(got, gt, u, unk, correct, (0.95,), (dtype.__name__, unk, "inf, zeros"))
            assert want["counts"][1] == int((gt == unk).sum()) and want["counts"][3] == 0
            other = gt == -3 - unk
            # dropping the other label's rows changes no integer; the two sums then run in the order of another N
            full, cut = detection_metrics(gt, u, unk_label=unk), detection_metrics(gt[~other], u[~other], unk_label=unk)
            for key in ("auroc", "fpr_at_tpr", "known", "unknown"):
                assert full[key] == cut[key], (key, unk)
            for key in ("aupr_in", "aupr_out"):
                assert abs(full[key] - cut[key]) <= 2 * SUM_RTOL * cut[key], (key, unk)
            raw, raw_cut = _detection_ranks(gt, u, unk_label=unk), _detection_ranks(gt[~other], u[~other], unk_label=unk)
            assert np.array_equal(raw["ranks"][:4, ~other], raw_cut["ranks"][:4]) and raw["counts"] == raw_cut["counts"]
        nan_rows = rng.permutation(N)[:25]
        v = u.copy(); v[nan_rows] = np.nan
        got = abi_run(cuda, gt, v, -2, correct, (0.95,))
        want = check_against_oracle(got, gt, v, -2, correct, (0.95,), (dtype.__name__, "nan"))
        assert want["counts"][3] == 25 and not got["ranks"][:, nan_rows].any()
        live = ~np.isnan(v)                                            # the other rows rank as if the NaN rows were not there
        assert np.array_equal(got["ranks"][:, live], O.ranks(gt[live], v[live], -2, correct[live])[0])
        with pytest.raises(ValueError, match="Input contains NaN"):
            detection_metrics(gt, v)
        assert _detection_ranks(gt, v)["counts"][3] == 25


def test_protocol_size(cuda):
    """N = 20000 with 40 % negatives: every integer and the curve against the oracle, the values against the oracle's exact quotients."""
    from openset_imagenet.metrics import detection_metrics
    rng = np.random.default_rng(20000)
    N = 20000
    gt = rng.integers(0, 116, size=N); gt[rng.random(N) < 0.4] = -2
    u = (np.round((rng.normal(size=N) + 1.0 * (gt < 0)) * 512) / 512).astype(np.float32)
    correct = (rng.random(N) < 0.7).astype(np.uint8)
    tpr = (0.9, 0.95)
    got = abi_run(cuda, gt, u, -2, correct, tpr)
    want = check_against_oracle(got, gt, u, -2, correct, tpr, "protocol")
    assert want["eq_pairs"] > 0 and 1000 < got["totals"][0] < want["counts"][0]
    m, ref = detection_metrics(gt, u, tpr=tpr), O.metrics(gt, u, -2, tpr)
    assert same_bits(m["auroc"], ref["auroc"]) and m["fpr_at_tpr"] == ref["fpr_at_tpr"]
    assert abs(m["aupr_in"] - ref["aupr_in"]) <= 1e-12 and abs(m["aupr_out"] - ref["aupr_out"]) <= 1e-12


def test_evaluate_main_detection(cuda, tmp_path):
    """script/evaluate.py --detection end to end on four JPEGs a split: a line and a JSON row for every scorer and negative label
    present, the figures those of detection_metrics / oscr_by_rejection on the arrays main() wrote."""
    import json
    from PIL import Image
    from openset_imagenet import ResNet50, tools
    from openset_imagenet.metrics import detection_metrics
    from openset_imagenet.script import evaluate
    from openset_imagenet.util import oscr_area, oscr_by_rejection
    tools.set_device_gpu(0)
    rng = np.random.default_rng(0)
    img_dir, proto, out = tmp_path / "imgs", tmp_path / "protocols", tmp_path / "out"
    for d in (img_dir, proto, out):
        d.mkdir()
    labels = {"train": (0, 1, 2, -1), "val": (0, 1, 2, -1), "test": (2, -2, 0, -1)}
    for split, ys in labels.items():
        for i, y in enumerate(ys):
            Image.fromarray(rng.integers(0, 256, size=(256, 256, 3), dtype=np.uint8)).save(img_dir / f"{split}_{i}.jpg", quality=90)
        (proto / f"p2_{split}.csv").write_text("".join(f"{split}_{i}.jpg,{y}\n" for i, y in enumerate(ys)))
    torch.manual_seed(3)
    torch.save({"epoch": 1, "model_state_dict": ResNet50(3, 3, False).state_dict(), "opt_state_dict": {}, "best_score": 0.5},
               out / "softmax_curr.pth")
    base = ["softmax", "2", "-g", "0", "--imagenet-directory", str(img_dir), "--protocol-directory", str(proto), "--output-directory",
            str(out), "--batch-size", "4", "--workers", "0"]
    written = evaluate.main(base + ["--detection", "--knn", "1", "--evm", "2", "--vim", "--vim-dim", "1"])
    assert sorted(written) == ["test", "test_detection", "test_evm", "test_knn", "test_vim", "val", "val_detection", "val_evm", "val_knn",
                               "val_vim"]
    scorers = ["MSP", "MaxLogit", "Energy", "EVM (-max score)", "KNN", "ViM"]
    for split, negatives in (("val", [-1]), ("test", [-1, -2])):
        report = json.load(open(written[f"{split}_detection"]))
        assert report["split"] == split and report["tpr"] == [0.95]
        assert [(r["scorer"], r["unk_label"]) for r in report["rows"]] == [(s, unk) for unk in negatives for s in scorers]
        knn, plain = dict(np.load(written[f"{split}_knn"])), dict(np.load(written[split]))
        for row in report["rows"]:
            assert "error" not in row and 0.0 <= row["auroc"] <= 1.0 and 0.0 <= row["fpr_at_tpr95"] <= 1.0
            if row["scorer"] == "KNN":
                m = detection_metrics(knn["gt"], knn["unknown"], unk_label=row["unk_label"])
                area = oscr_area(*oscr_by_rejection(knn["gt"], knn["scores"], knn["unknown"], unk_label=row["unk_label"]))
                assert (row["auroc"], row["aupr_in"], row["aupr_out"], row["fpr_at_tpr95"]) == (m["auroc"], m["aupr_in"], m["aupr_out"], m["fpr_at_tpr"][0])
                assert row["oscr_area"] == area and row["known"] == int((plain["gt"] >= 0).sum())
            if row["scorer"] == "MaxLogit":
                assert row["auroc"] == detection_metrics(plain["gt"], -plain["logits"].max(1), unk_label=row["unk_label"])["auroc"]
        assert evaluate.detection_line(split, report["rows"][0]).startswith(f"{split}: detection MSP vs label -1: AUROC ")

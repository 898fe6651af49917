"""CPU side of the ROC-AUC mirror (metrics.auc_score_binary / auc_score_multiclass, reference metrics.py:65-106): the names import
without a GPU and refuse to run there, the C ABI entries validate their arguments before any launch, and the fixture produced by the
reference's own functions (tests/golden/make_golden_auc.py) is what an exact pair count says it is.

The exact-count oracle of this file (np.sort + searchsorted, then the host expression of metrics.py) is also what the GPU tests
(tests/test_auc_gpu.py) compare against, bit for bit."""
import os

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------------------------- oracle
def pair_counts(pos, neg):
    """Exact (#{p > n}, #{p == n}) over all pairs of two 1-D arrays, as Python ints."""
    srt = np.sort(neg)
    lo = np.searchsorted(srt, pos, side="left")
    hi = np.searchsorted(srt, pos, side="right")
    return int(lo.sum(dtype=np.int64)), int((hi - lo).sum(dtype=np.int64))


def mann_whitney(gt, eq, P, Nn):
    return (2 * gt + eq) / (2 * P * Nn) if P and Nn else float("nan")


def oracle_binary(target_labels, pred_scores, unk_class=-1):
    y, s = np.asarray(target_labels), np.asarray(pred_scores)
    m = s.max(axis=1)
    known = y != unk_class
    g, e = pair_counts(m[known], m[~known])
    return mann_whitney(g, e, int(known.sum()), int((~known).sum()))


def oracle_multiclass(target_labels, pred_scores):
    y, s = np.asarray(target_labels), np.asarray(pred_scores)
    a = []
    for c in range(s.shape[1]):
        p = y == c
        g, e = pair_counts(s[p, c], s[~p, c])
        a.append(mann_whitney(g, e, int(p.sum()), int((~p).sum())))
    return float(np.mean(np.asarray(a, dtype=np.float64)))


def load_cases(golden_dir):
    """The fixture as a list of dicts: name, kind, gt, scores, unk, auc, refused."""
    G = np.load(os.path.join(golden_dir, "auc_reference.npz"))
    return [dict(name=str(n), kind=str(G[f"{n}.kind"]), gt=G[f"{n}.gt"], scores=G["scores." + str(G[f"{n}.scores_id"])],
                 unk=int(G[f"{n}.unk"]), auc=float(G[f"{n}.auc"]), refused=bool(G[f"{n}.refused"])) for n in G["names"]]


# ----------------------------------------------------------------------------------------------------------------- tests
def test_names_import_and_refuse_without_gpu():
    from openset_imagenet.metrics import auc_score_binary, auc_score_multiclass, confidence  # noqa: F401  (the reference's train.py:16)
    gt, s = np.array([0, 1, 0, 1]), np.array([[0.75, 0.25], [0.5, 0.5], [0.25, 0.75], [0.125, 0.875]], dtype=np.float32)
    for fn in (auc_score_binary, auc_score_multiclass):
        if torch.cuda.is_available():                    # with a GPU present they simply answer
            assert 0.0 <= fn(gt, s, **({"unk_class": 1} if fn is auc_score_binary else {})) <= 1.0
        else:
            with pytest.raises(RuntimeError, match="no CPU path"):
                fn(gt, s)


def test_abi_entries_validate_before_launch():
    """Null pointers, N = 0, C = 0, a short workspace and (one-vs-rest) a row wider than the LDS tiling: OSI_ERR_ARG, nothing launched
    (safe on a CPU-only host; the pointers are never dereferenced on the host)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 16
    assert lib.osi_auc_workspace(0) == 0 and lib.osi_auc_workspace(-3) == 0
    nb = lib.osi_auc_workspace(100)
    assert nb >= 100 * 8
    p = 4096                                             # any non-null address: argument checks come first
    for fn in (lib.osi_auc_binary_f32, lib.osi_auc_binary_f64):
        assert fn(None, p, 100, 4, -1, p, nb, p, None) == -1
        assert fn(p, None, 100, 4, -1, p, nb, p, None) == -1
        assert fn(p, p, 100, 4, -1, None, nb, p, None) == -1
        assert fn(p, p, 100, 4, -1, p, nb, None, None) == -1
        assert fn(p, p, 0, 4, -1, p, nb, p, None) == -1
        assert fn(p, p, 100, 0, -1, p, nb, p, None) == -1
        assert fn(p, p, 100, 4, -1, p, nb - 1, p, None) == -1
    for fn in (lib.osi_auc_ovr_f32, lib.osi_auc_ovr_f64):
        for hole in (0, 1, 4, 6, 7, 8, 9):               # every pointer argument in turn
            args = [p, p, 100, 4, p, nb, p, p, p, p, None]
            args[hole] = None
            assert fn(*args) == -1, hole
        assert fn(p, p, 0, 4, p, nb, p, p, p, p, None) == -1
        assert fn(p, p, 100, 0, p, nb, p, p, p, p, None) == -1
        assert fn(p, p, 100, 4, p, nb - 1, p, p, p, p, None) == -1
        assert fn(p, p, 100, 2049, p, nb, p, p, p, p, None) == -1


def test_fixture_is_the_exact_pair_count(golden_dir):
    """Every value the reference returned (sklearn 1.7.2's trapezoid sum over the sorted thresholds) is the Mann-Whitney quotient of
    exact integer pair counts within 1e-12 absolute. Worst case seen when the fixture was generated: 1.1e-16 (printed below); the
    bar is four orders above it. nan cases are nan on both sides; refusal cases carry no value."""
    cases = load_cases(golden_dir)
    assert sum(c["kind"] == "binary" for c in cases) >= 10 and sum(c["kind"] == "multiclass" for c in cases) >= 8
    assert sum(c["refused"] for c in cases) == 3
    worst = 0.0
    for c in cases:
        if c["refused"]:
            assert np.isnan(c["auc"])
            continue
        got = oracle_binary(c["gt"], c["scores"], c["unk"]) if c["kind"] == "binary" else oracle_multiclass(c["gt"], c["scores"])
        if np.isnan(c["auc"]):
            assert np.isnan(got), c["name"]
            continue
        worst = max(worst, abs(got - c["auc"]))
        assert abs(got - c["auc"]) <= 1e-12, (c["name"], got, c["auc"])
    print(f"largest |oracle - reference| over the fixture: {worst:.3e}")
    by = {c["name"]: c for c in cases}
    assert by["bin_all_equal"]["auc"] == 0.5
    assert np.isnan(by["bin_only_positives"]["auc"]) and np.isnan(by["bin_only_negatives"]["auc"]) and np.isnan(by["bin_one_row"]["auc"])
    assert {-1, -2} <= set(by["bin_unk_minus2"]["gt"].tolist()) and by["bin_unk_minus2"]["unk"] == -2
    assert np.bincount(by["mc_class_with_one_sample"]["gt"]).min() == 1

"""CPU side of the detection metrics (metrics.detection_metrics, util.oscr_by_rejection, csrc/detection.hip; include/osi.h, ABI 28):
the numpy oracle (tests/detection_oracle.py) against the values sklearn gave (tests/golden/make_golden_detection.py), the names import
and refuse without a GPU, the C ABI entries validate their arguments before any launch, and evaluate.py knows `--detection`."""
import numpy as np
import pytest
import torch

import detection_oracle as O


def test_oracle_matches_the_sklearn_fixture(golden_dir):
    """AUROC, AUPR-in, AUPR-out within 1e-12 of sklearn 1.7.2 (the bar of the AUC fixture; the oracle rounds exact quotients once, and
    sklearn's own sums are good to a few ulp), FPR at TPR equal within the same bar (both are one division of the same integers)."""
    cases = O.load_cases(golden_dir)
    assert len(cases) >= 15 and max(len(c["gt"]) for c in cases) <= 2000
    by = {c["name"]: c for c in cases}
    worst = 0.0
    for c in cases:
        if c["refused"]:
            with pytest.raises(ValueError, match="NaN"):
                O.metrics(c["gt"], c["u"], c["unk"], c["tpr"])
            continue
        got = O.metrics(c["gt"], c["u"], c["unk"], c["tpr"])
        pairs = [(got[k], c[k]) for k in ("auroc", "aupr_in", "aupr_out")] + list(zip(got["fpr_at_tpr"], c["fpr_at_tpr"]))
        assert len(got["fpr_at_tpr"]) == len(c["tpr"])
        for mine, ref in pairs:
            if np.isnan(ref):
                assert np.isnan(mine), c["name"]
            else:
                worst = max(worst, abs(mine - ref))
                assert abs(mine - ref) <= 1e-12, (c["name"], mine, ref)
    print(f"largest |oracle - sklearn| over the fixture: {worst:.3e}")
    assert sum(c["refused"] for c in cases) == 1 and np.isnan(by["nan_refused"]["u"]).any()
    assert by["all_tied"]["auroc"] == 0.5 and by["all_tied"]["fpr_at_tpr"] == [1.0, 1.0]
    assert np.isnan(by["only_known"]["auroc"]) and np.isnan(by["only_unknown"]["aupr_in"]) and np.isnan(by["one_row"]["auroc"])
    assert np.isposinf(by["infinities"]["u"]).any() and np.isneginf(by["infinities"]["u"]).any()
    assert {-1, -2} <= set(by["minus1_beside_minus2"]["gt"].tolist()) and by["minus1_beside_minus2"]["unk"] == -2
    assert by["unk_minus1"]["unk"] == -1 and by["inverted"]["auroc"] < 0.5
    z = by["signed_zeros"]["u"]
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    ties = O.summary(by["ties_f32"]["gt"], by["ties_f32"]["u"], -2)
    assert ties["eq_pairs"] > 0


def test_oracle_curve_is_calculate_oscr_with_negated_confidence():
    """The curve by rejection with u = -max score and every known row correct, against the definition of util.calculate_oscr
    (reference util.py:90-122) written out in numpy."""
    rng = np.random.default_rng(5)
    N, C = 300, 6
    gt = rng.integers(0, C, size=N); gt[rng.random(N) < 0.4] = -1
    s = np.round(rng.random((N, C)) * 8) / 16
    kn_rows = np.flatnonzero(gt >= 0)
    s[kn_rows, gt[kn_rows]] = 0.5625 + np.round(rng.random(len(kn_rows)) * 7) / 16           # the label column wins: every known row correct
    assert O.first_max_correct(gt, s)[gt >= 0].all()
    ccr, fpr = O.oscr_by_rejection(gt, s, -s.max(1), unk_label=-1)
    kn, un = gt >= 0, gt == -1
    tgt = s[kn, gt[kn]]
    taus = np.unique(tgt)[:-1]
    want_ccr = np.array([np.sum(tgt > t) for t in taus]) / kn.sum()
    want_fpr = np.array([np.sum(s[un].max(1) > t) for t in taus]) / un.sum()
    assert len(taus) < kn.sum() and np.array_equal(ccr, want_ccr) and np.array_equal(fpr, want_fpr)


def test_names_import_and_refuse_without_gpu():
    from openset_imagenet.metrics import _detection_ranks, detection_metrics
    from openset_imagenet.util import oscr_area, oscr_by_rejection
    gt, u = np.array([0, 1, -2, -2]), np.array([0.25, 0.5, 0.5, 0.75], dtype=np.float32)
    s = np.array([[0.75, 0.25], [0.25, 0.75], [0.5, 0.5], [0.5, 0.5]], dtype=np.float32)
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert detection_metrics(gt, u)["auroc"] == 0.875
        assert len(oscr_by_rejection(gt, s, u, unk_label=-2)[0]) == 1
    else:
        for call in (lambda: detection_metrics(gt, u), lambda: _detection_ranks(gt, u), lambda: oscr_by_rejection(gt, s, u)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
    with pytest.raises(ValueError, match="tpr"):
        detection_metrics(gt, u, tpr=())
    with pytest.raises(ValueError, match="tpr"):
        detection_metrics(gt, u, tpr=(0.0,))
    # the area is host arithmetic: a falling-fpr curve, no extrapolation
    assert oscr_area(np.array([0.5, 0.25, 0.0]), np.array([1.0, 0.5, 0.0])) == 0.25
    assert oscr_area(np.zeros(1), np.zeros(1)) == 0.0 and np.isnan(oscr_area(np.array([np.nan, 0.0]), np.array([1.0, 0.0])))


def test_abi_entries_validate_before_launch():
    """Each null required pointer, N = 0, unk_label = 0, Q = 0, Q = 9 and a workspace one byte short: OSI_ERR_ARG, nothing launched
    (safe on a CPU-only host; the pointers are never dereferenced on the host). `correct` is the one optional pointer."""
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 28
    assert lib.osi_det_workspace(0) == 0 and lib.osi_det_workspace(-3) == 0 and lib.osi_det_workspace(2 ** 31 - 1) == 0
    nb = lib.osi_det_workspace(100)
    assert nb >= 100 * 16
    p = 4096                                             # any non-null address: argument checks come first

    def refuses(fn, args, pointers, n_at, unk_at, ws_at):
        for hole in pointers:
            bad = list(args); bad[hole] = None
            assert fn(*bad) == -1, (fn.__name__, hole)
        for at, value in ((n_at, 0), (n_at, -5), (unk_at, 0), (unk_at, 3), (ws_at, nb - 1)):
            bad = list(args); bad[at] = value
            assert fn(*bad) == -1, (fn.__name__, at, value)

    for fn in (lib.osi_det_ranks_f32, lib.osi_det_ranks_f64):
        refuses(fn, [p, p, None, 100, -2, p, nb, p, p, None], (0, 1, 5, 7, 8), 3, 4, 6)
        refuses(fn, [p, p, p, 100, -1, p, nb, p, p, None], (0, 1, 5, 7, 8), 3, 4, 6)
    summary = [p, p, 100, -2, p, 1, p, nb, p, p, None]
    refuses(lib.osi_det_summary, summary, (0, 1, 4, 6, 8, 9), 2, 3, 7)
    for q in (0, 9, -1):
        bad = list(summary); bad[5] = q
        assert lib.osi_det_summary(*bad) == -1, q
    for fn in (lib.osi_det_curve_f32, lib.osi_det_curve_f64):
        refuses(fn, [p, p, p, 100, -2, p, nb, p, p, p, p, None], (0, 1, 2, 5, 7, 8, 9, 10), 3, 4, 6)


def test_get_args_accepts_detection():
    from openset_imagenet.script.evaluate import get_args
    assert get_args(["entropic", "1"]).detection is False
    args = get_args(["entropic", "1", "--detection", "--vim", "--knn", "10"])
    assert args.detection and args.vim and args.knn == 10

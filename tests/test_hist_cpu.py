"""CPU side of the evaluation histograms (util.get_histogram, reference util.py:202-228; util.nearest_fpr / ccr_at_fpr, reference
script/plot_all.py:344-385): the names import without a GPU and refuse to run there, the C ABI entries validate their arguments
before any launch, the fixture produced by the reference's own function (tests/golden/make_golden_hist.py) is what an exact
restatement of np.histogram says it is, and the host-only FPR rule picks what the reference's table picks.

The oracle of this file (searchsorted over the fp64 edges, last bin closed, outside values dropped) is also what the GPU tests
(tests/test_hist_gpu.py) compare against, count for count."""
import os

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------------------------- oracle
def oracle_hist(x, edges):
    """np.histogram's counts for explicit edges, restated: bin = searchsorted(edges, x, 'right') - 1 in fp64, x == edges[-1] in the
    last bin, NaN and values outside [edges[0], edges[-1]] dropped."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    nb = len(e) - 1
    with np.errstate(invalid="ignore"):
        x = x[(x >= e[0]) & (x <= e[-1])]
    return np.bincount(np.minimum(np.searchsorted(e, x, side="right") - 1, nb - 1), minlength=nb).astype(np.int64)


def host_norms(features):
    """Row norms as the device forms them: fp64 squares, fp64 sum, one fp64 sqrt, one rounding to the features' dtype."""
    f = np.asarray(features)
    return np.sqrt((f.astype(np.float64) ** 2).sum(1)).astype(f.dtype)


def side_values(scores, features, gt, unk_label, metric, drop_bg):
    """(kn_metric, unk_metric) of util.py:209-222, restated with numpy."""
    gt = np.asarray(gt).astype(np.int64)
    kn, unk = gt >= 0, gt == unk_label
    if metric == "norm":
        n = host_norms(features)
        return n[kn], n[unk]
    s = scores[:, :-1] if drop_bg else scores
    return s[kn, gt[kn]], np.amax(s[unk], axis=1)


def host_edges(x, bins):
    """The rule util.get_histogram forms its edges by, from {min, max} alone."""
    if len(x) == 0:
        return np.histogram_bin_edges(np.empty(0, dtype=x.dtype), bins)
    return np.histogram_bin_edges(np.array([x.min(), x.max()], dtype=x.dtype), bins)


def load_cases(golden_dir):
    """The fixture as a list of dicts (tests/golden/make_golden_hist.py describes the layout)."""
    G = np.load(os.path.join(golden_dir, "hist_reference.npz"))
    out = []
    for n in G["names"]:
        s = G["scores." + str(G[f"{n}.scores_id"])]
        f = G["features." + str(G[f"{n}.features_id"])][:len(s)]
        out.append(dict(name=str(n), scores=s, features=f, gt=G[f"{n}.gt"], unk=int(G[f"{n}.unk"]), metric=str(G[f"{n}.metric"]),
                        bins=int(G[f"{n}.bins"]), drop_bg=bool(G[f"{n}.drop_bg"]), log_space=bool(G[f"{n}.log_space"]),
                        limits=tuple(G[f"{n}.limits"].tolist()), refused=int(G[f"{n}.refused"]),
                        want=tuple(G[f"{n}.{k}"] for k in ("kn_hist", "kn_edges", "unk_hist", "unk_edges"))))
    return out


def fpr_rule(ccr, fpr, q, max_error=10.0):
    """plot_all.py:346-384 for one query, restated."""
    if len(fpr) == 0:
        return None
    idx = np.abs(np.asarray(fpr) - q).argmin()
    return None if round(100 * abs(fpr[idx] - q) / q, 1) >= max_error else ccr[idx]


# ----------------------------------------------------------------------------------------------------------------- tests
def test_names_import_and_refuse_without_gpu():
    from openset_imagenet.util import ccr_at_fpr, get_histogram, nearest_fpr  # noqa: F401
    from openset_imagenet.script.evaluate import evaluation_report  # noqa: F401
    gt = np.array([0, 1, -1, -2, 1])
    s = np.array([[0.75, 0.25], [0.5, 0.5], [0.25, 0.75], [0.125, 0.875], [0.25, 0.75]], dtype=np.float32)
    arr = dict(scores=s, gt=gt, features=np.ones((5, 3), dtype=np.float32))
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert get_histogram(arr, bins=4)[0].sum() == 3
        assert len(ccr_at_fpr(gt, s)) == 4
    else:
        for call in (lambda: get_histogram(arr), lambda: get_histogram(arr, metric="norm"), lambda: ccr_at_fpr(gt, s),
                     lambda: evaluation_report(gt, s, arr["features"], "entropic")):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
    # decided on the host, before anything else
    with pytest.raises(ValueError, match="metric"):
        get_histogram(arr, metric="angle")
    with pytest.raises(ValueError, match="4096"):
        get_histogram(arr, bins=4097)
    with pytest.raises(ValueError, match="4096"):
        get_histogram(arr, bins=np.linspace(0, 1, 4098))
    with pytest.raises(ValueError, match="monotonically"):
        get_histogram(arr, bins=[0.0, 0.5, 0.25, 1.0])
    with pytest.raises(ValueError, match="positive"):
        get_histogram(arr, bins=0)


def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 18
    for name in ("osi_eval_values_workspace", "osi_eval_values_f32", "osi_eval_values_f64", "osi_hist_f32", "osi_hist_f64"):
        assert hasattr(lib, name) and name in N.declared_symbols()
    assert (N.EVAL_SCORE, N.EVAL_NORM, N.HIST_MAX_BINS) == (0, 1, 4096)


def test_abi_entries_validate_before_launch():
    """Null pointers, N = 0, nb of 0 and 4097, a short workspace, a bad metric, no class column: OSI_ERR_ARG, nothing launched (safe
    on a CPU-only host; the pointers are never dereferenced on the host)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_eval_values_workspace(0) == 0 and lib.osi_eval_values_workspace(-3) == 0
    nb = lib.osi_eval_values_workspace(100)
    assert nb > 0
    p = 4096                                             # any non-null address: argument checks come first
    for fn in (lib.osi_eval_values_f32, lib.osi_eval_values_f64):
        good = [p, p, p, 100, 4, 5, N.EVAL_SCORE, -1, 0, p, p, p, p, p, p, nb, None]
        for hole in (2, 9, 10, 11, 12, 13, 14):          # every pointer both metrics need
            args = list(good); args[hole] = None
            assert fn(*args) == -1, hole
        for metric, hole in ((N.EVAL_SCORE, 0), (N.EVAL_NORM, 1)):     # the matrix the metric reads
            args = list(good); args[6] = metric; args[hole] = None
            assert fn(*args) == -1, (metric, hole)
        for pos, value in ((3, 0), (3, -5), (15, nb - 1), (6, 2), (6, -1), (8, 2)):   # N, workspace, metric, drop_last
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (pos, value)
        args = list(good); args[4] = 1; args[8] = 1      # one column, and that one the background
        assert fn(*args) == -1
        args = list(good); args[6] = N.EVAL_NORM; args[5] = 0
        assert fn(*args) == -1
    for fn in (lib.osi_hist_f32, lib.osi_hist_f64):
        good = [p, p, 1, 100, p, 30, p, None]
        for hole in (0, 1, 4, 6):
            args = list(good); args[hole] = None
            assert fn(*args) == -1, hole
        for pos, value in ((3, 0), (3, -1), (5, 0), (5, 4097), (5, -1), (2, 0), (2, 256)):   # N, nb, side_bit
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (pos, value)
        args = list(good); args[0] = p + 2               # a value pointer off its element size
        assert fn(*args) == -1


def test_fixture_is_the_exact_restatement(golden_dir):
    """Every histogram the reference returned is the oracle's over the reference's own edges, those edges are what numpy makes of
    {min, max} alone (integer bins) or np.geomspace (log_space), dtypes included, and the refusals are the three planned ones."""
    cases = load_cases(golden_dir)
    assert len(cases) >= 14
    assert {c["name"] for c in cases if c["refused"] == 1} == {"drop_bg_label_is_bg"}
    assert {c["name"] for c in cases if c["refused"] == 2} == {"nan_score"}
    assert {np.float32, np.float64} == {c["scores"].dtype.type for c in cases}
    assert {1, 30, 100} <= {c["bins"] for c in cases} and {-1, -2} == {c["unk"] for c in cases}
    for c in cases:
        assert c["scores"].shape[0] <= 600 and c["scores"].shape[1] <= 12
        if c["refused"]:
            continue
        kn_hist, kn_edges, unk_hist, unk_edges = c["want"]
        kn, unk = side_values(c["scores"], c["features"], c["gt"], c["unk"], c["metric"], c["drop_bg"])
        assert kn_hist.dtype == np.int64 and unk_hist.dtype == np.int64
        assert np.array_equal(kn_hist, oracle_hist(kn, kn_edges)), c["name"]
        assert np.array_equal(unk_hist, oracle_hist(unk, unk_edges)), c["name"]
        if c["log_space"]:
            want = np.geomspace(*c["limits"], num=c["bins"])
            assert len(kn_edges) == c["bins"] and kn_edges.dtype == np.float64
            assert np.array_equal(kn_edges, want) and np.array_equal(unk_edges, want)
        else:
            for x, e in ((kn, kn_edges), (unk, unk_edges)):
                w = host_edges(x, c["bins"])
                assert e.dtype == w.dtype == x.dtype and np.array_equal(e, w), c["name"]
    by = {c["name"]: c for c in cases}
    assert by["no_unknown_rows"]["want"][2].sum() == 0 and by["no_unknown_rows"]["want"][3][[0, -1]].tolist() == [0.0, 1.0]
    assert by["no_known_rows"]["want"][0].sum() == 0
    one = by["one_unknown_row"]["want"]
    assert one[2].sum() == 1 and one[3][-1] - one[3][0] == 1.0                  # a single value: the range widens by +-0.5
    eq = by["equal_values"]["want"]
    assert np.count_nonzero(eq[0]) == 1 and np.float32(eq[1][-1] - eq[1][0]) == 1.0
    q = by["quantised_bins32"]
    assert q["want"][1][[0, -1]].tolist() == [0.0, 1.0]                         # k/64 values on edges k/32
    assert np.isin(side_values(q["scores"], None, q["gt"], -1, "score", False)[0], q["want"][1]).sum() > 20
    assert by["drop_bg_ok"]["gt"].max() == by["drop_bg_ok"]["scores"].shape[1] - 2
    assert by["drop_bg_label_is_bg"]["gt"].max() == by["drop_bg_label_is_bg"]["scores"].shape[1] - 1
    assert by["gt_as_float32"]["gt"].dtype == np.float32
    for n in ("norm_f32_bins30", "norm_f64_bins100"):                           # integer-valued features: the norms are the same bits
        f = by[n]["features"]
        assert np.array_equal(f, np.round(f)) and np.abs(f).max() <= 3
        assert np.array_equal(np.linalg.norm(f, axis=1), host_norms(f))


def test_nearest_fpr_is_the_table_rule():
    from openset_imagenet.util import nearest_fpr
    # exact hits; the nearest point to 1.0 is 50 % off
    ccr, fpr = np.array([0.9, 0.8, 0.7, 0.6]), np.array([0.5, 0.1, 0.01, 0.001])
    assert nearest_fpr(ccr, fpr) == [0.6, 0.7, 0.8, None]
    # two points equally far (dyadic, so exactly): the first one
    ccr, fpr = np.array([0.25, 0.75, 0.5]), np.array([0.515625, 0.484375, 0.75])
    assert nearest_fpr(ccr, fpr, fpr_values=(0.5,)) == [0.25]
    assert nearest_fpr(ccr[::-1], fpr[::-1], fpr_values=(0.5,)) == [0.75]
    # the boundary: the percentage is rounded to one decimal first, 9.9 passes and what rounds to 10.0 does not
    for f, kept in ((0.901, True), (0.9006, True), (0.9004, False), (0.9, False), (1.099, True), (1.1, False)):
        got = nearest_fpr(np.array([0.375]), np.array([f]), fpr_values=(1.0,))
        assert got == ([0.375] if kept else [None]), f
        assert got == [fpr_rule([0.375], [f], 1.0)]
    assert nearest_fpr(np.array([0.375]), np.array([0.8]), fpr_values=(1.0,), max_error=25.0) == [0.375]
    # an empty curve: nothing to pick (the reference would raise)
    assert nearest_fpr(np.zeros(0), np.zeros(0)) == [None] * 4
    assert nearest_fpr([], [], fpr_values=(0.1,)) == [None]
    # a NaN in fpr: argmin lands on it and the NaN error is not >= the bar, so the rule hands out that point's ccr
    ccr, fpr = np.array([0.5, 0.625, 0.75]), np.array([0.2, np.nan, 0.1])
    assert nearest_fpr(ccr, fpr) == [0.625] * 4 == [fpr_rule(ccr, fpr, q) for q in (1e-3, 1e-2, 0.1, 1.0)]
    # random curves against the restated rule
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(1, 40))
        ccr, fpr = rng.random(n), np.sort(rng.random(n) ** 3)[::-1]
        assert nearest_fpr(ccr, fpr) == [fpr_rule(ccr, fpr, q) for q in (1e-3, 1e-2, 0.1, 1.0)]

"""GPU parity of the evaluation histograms (util.get_histogram, csrc/hist.hip; util.ccr_at_fpr; script.evaluate.evaluation_report):
the arrays the reference's own get_histogram returned (tests/golden/hist_reference.npz) and the counts of the exact numpy oracle of
tests/test_hist_cpu.py. Everything the device produces here is an integer count or a stored value: exact equality everywhere."""
import numpy as np
import pytest
import torch

from test_hist_cpu import fpr_rule, host_norms, load_cases, oracle_hist, side_values

pytestmark = pytest.mark.gpu

GARBAGE = -7777                                            # what the output buffers hold before a call


# ------------------------------------------------------------------------------------------------------- fixture, public API
def test_fixture_cases_host_and_device_inputs(cuda, golden_dir):
    from openset_imagenet.util import get_histogram
    for c in load_cases(golden_dir):
        for where in ("host", "device"):
            arr = dict(scores=c["scores"].copy(), gt=c["gt"].copy(), features=c["features"].copy())
            if where == "device":
                arr = {k: torch.from_numpy(v).to(cuda) for k, v in arr.items()}
            call = lambda: get_histogram(arr, unk_label=c["unk"], metric=c["metric"], bins=c["bins"], drop_bg=c["drop_bg"],
                                         log_space=c["log_space"], geomspace_limits=c["limits"])
            if c["refused"]:
                with pytest.raises(IndexError if c["refused"] == 1 else ValueError):
                    call()
                continue
            got = call()
            for g, w, key in zip(got, c["want"], ("kn_hist", "kn_edges", "unk_hist", "unk_edges")):
                assert isinstance(g, np.ndarray) and g.dtype == w.dtype, (c["name"], where, key, g.dtype, w.dtype)
                assert np.array_equal(g, w), (c["name"], where, key)
            back = {k: (v.cpu().numpy() if where == "device" else v) for k, v in arr.items()}     # inputs are never written
            assert all(np.array_equal(back[k], c[k], equal_nan=True) for k in ("scores", "gt", "features")), (c["name"], where)


def test_public_refusals_and_edge_sequences(cuda):
    from openset_imagenet.util import get_histogram
    rng = np.random.default_rng(9)
    s = rng.random((300, 6)).astype(np.float32)
    gt = rng.integers(-2, 6, size=300)
    arr = dict(scores=s, gt=gt)                              # no features: only metric='norm' reads them
    kn, unk = side_values(s, None, gt, -1, "score", False)
    edges = [0.0, 0.25, 0.25, 0.5, 1.0, 1.0]                 # a sequence: explicit edges, repeated ones included
    kh, ke, uh, ue = get_histogram(arr, bins=edges)
    assert np.array_equal(kh, np.histogram(kn, bins=edges)[0]) and np.array_equal(uh, np.histogram(unk, bins=edges)[0])
    assert ke.dtype == np.float64 and np.array_equal(ke, edges) and np.array_equal(ue, edges)
    with pytest.raises(KeyError):
        get_histogram(arr, metric="norm")
    inf = s.copy(); inf[np.flatnonzero(gt == -1)[0], 2] = np.inf
    with pytest.raises(ValueError, match="is not finite"):
        get_histogram(dict(scores=inf, gt=gt), bins=30)
    kh2, _, uh2, _ = get_histogram(dict(scores=inf, gt=gt), bins=edges)          # explicit edges: the infinity is just outside
    assert np.array_equal(kh2, kh) and uh2.sum() == uh.sum() - 1
    # float16 scores are cast to fp64, as calculate_oscr does
    s16 = s.astype(np.float16)
    kn16, unk16 = side_values(s16.astype(np.float64), None, gt, -2, "score", False)
    got = get_histogram(dict(scores=s16, gt=gt), unk_label=-2, bins=30)
    for g, w in zip(got, np.histogram(kn16, bins=30) + np.histogram(unk16, bins=30)):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    # no rows at all
    kh, ke, uh, ue = get_histogram(dict(scores=np.zeros((0, 4), np.float32), gt=np.zeros(0)), bins=5)
    want = np.histogram(np.zeros(0, np.float32), bins=5)
    for g, w in zip((kh, ke, uh, ue), want + want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert ke.dtype == np.float32 and ke[[0, -1]].tolist() == [0.0, 1.0]


# ----------------------------------------------------------------------------------------------------------- osi_hist_*
def run_hist(cuda, val, side, bit, edges, offset=0):
    """osi_hist_* on copies of the arrays; `offset` elements of padding in front put the values off the 16-byte boundary."""
    from openset_imagenet import _native as N
    lib = N.lib()
    pad = np.full(offset, 0.5, dtype=val.dtype)
    v = torch.from_numpy(np.concatenate([pad, val])).to(cuda)[offset:]
    sd = torch.from_numpy(np.concatenate([np.full(offset, 3, np.uint8), side])).to(cuda)[offset:]
    e = torch.from_numpy(np.asarray(edges, dtype=np.float64)).to(cuda)
    nb = len(edges) - 1
    counts = torch.full((nb + 1,), GARBAGE, dtype=torch.int64, device=cuda)      # one guard word behind the nb counters
    fn = lib.osi_hist_f32 if val.dtype == np.float32 else lib.osi_hist_f64
    N.check(fn(N.ptr(v), N.ptr(sd), bit, len(val), N.ptr(e), nb, N.ptr(counts), N.stream_of(v)), "osi_hist")
    out = counts.cpu().numpy()
    assert out[nb] == GARBAGE
    return out[:nb]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nb", [1, 2, 31, 100, 4096])
def test_hist_kernel_against_the_oracle(cuda, dtype, nb):
    """Values on edges, one ulp either side of them, below and above the range, NaN and +-inf, every value in one bin, a table with
    repeated edges, alternating and all-clear side masks, value pointers on and off the 16-byte boundary; counts pre-filled."""
    rng = np.random.default_rng(1000 + nb)
    plain = np.linspace(0, 1, nb + 1).astype(dtype)                              # edges the value type holds exactly
    repeated = plain.copy()
    repeated[-1] = repeated[-2] if nb > 1 else repeated[-1]                      # a zero-width LAST bin: x == edges[nb] still lands in it
    if nb > 4:
        repeated[3] = repeated[2]; repeated[nb // 2 + 1] = repeated[nb // 2 - 1] = repeated[nb // 2]
    big = np.finfo(dtype).max
    for n_i, N in enumerate((1, 3, 255, 257, 3001)):
        for table in (plain, repeated):
            pool = np.concatenate([table, np.nextafter(table, dtype(2)), np.nextafter(table, dtype(-1)),
                                   np.array([-1.0, -0.25, 1.5, big, -big, np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=dtype),
                                   rng.uniform(-0.05, 1.05, size=64).astype(dtype)])
            top = np.full(N, table[-1] if n_i % 2 else np.nextafter(table[-1], dtype(-1)), dtype=dtype)
            for val in (rng.choice(pool, size=N).astype(dtype), top):
                side = (1 + (np.arange(N) % 2) + 4 * rng.integers(0, 2, size=N)).astype(np.uint8)     # bits 0 / 1 alternate, bit 2 is noise
                offset = (n_i + nb) % 4 if dtype == np.float32 else (n_i + nb) % 2
                for bit in (1, 2):
                    want = oracle_hist(val[(side & bit) != 0], table)
                    got = run_hist(cuda, val, side, bit, table, offset)
                    assert np.array_equal(got, want), (N, nb, bit, offset, np.flatnonzero(got != want)[:5])
                assert not run_hist(cuda, val, side & 4, 3, table, offset).any()                      # no row takes part
            assert run_hist(cuda, top, np.full(N, 1, np.uint8), 1, table).sum() == N                  # one bin holds them all
    # an unsorted table: counts unspecified, but every one of them inside the table and nothing written behind it
    wild = rng.permutation(plain)
    wild[0], wild[-1] = plain[0], plain[-1]
    val = rng.uniform(0, 1, size=3001).astype(dtype)
    got = run_hist(cuda, val, np.full(3001, 1, np.uint8), 1, wild)
    assert got.min() >= 0 and got.sum() == 3001


# ------------------------------------------------------------------------------------------------------ osi_eval_values_*
def run_values(cuda, scores, features, gt, metric, unk_label, drop_last):
    """osi_eval_values_* with every output pre-filled: (kn_val, unk_val, side, range4, counts6) as numpy."""
    from openset_imagenet import _native as N
    lib = N.lib()
    src = scores if metric == N.EVAL_SCORE else features
    n, tdt = len(src), torch.float32 if src.dtype == np.float32 else torch.float64
    dev = lambda a: None if a is None else torch.from_numpy(a).to(cuda)
    s, f, y = dev(scores), dev(features), dev(gt.astype(np.int64))
    nb = lib.osi_eval_values_workspace(n)
    ws = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    kn, unk = torch.full((n,), float(GARBAGE), dtype=tdt, device=cuda), torch.full((n,), float(GARBAGE), dtype=tdt, device=cuda)
    side = torch.full((n,), 0xFF, dtype=torch.uint8, device=cuda)
    rng4 = torch.full((4,), float(GARBAGE), dtype=torch.float64, device=cuda)
    cnt6 = torch.full((6,), GARBAGE, dtype=torch.int64, device=cuda)
    fn = lib.osi_eval_values_f32 if tdt == torch.float32 else lib.osi_eval_values_f64
    N.check(fn(N.ptr(s), N.ptr(f), N.ptr(y), n, 0 if scores is None else scores.shape[1], 0 if features is None else features.shape[1],
               metric, unk_label, drop_last, N.ptr(kn), N.ptr(unk), N.ptr(side), N.ptr(rng4), N.ptr(cnt6), N.ptr(ws), nb,
               N.stream_of(y)), "osi_eval_values")
    return kn.cpu().numpy(), unk.cpu().numpy(), side.cpu().numpy(), rng4.cpu().numpy(), cnt6.cpu().numpy()


def check_values(got, kn_val, unk_val, known, unk, bad, what):
    """Values (one expected entry per row), side bytes, range4 and counts6 against numpy's; the range of a side without a non-NaN
    value is not read."""
    g_kn, g_unk, g_side, g_rng, g_cnt = got
    assert np.array_equal(g_kn, kn_val, equal_nan=True), what
    assert np.array_equal(g_unk, unk_val, equal_nan=True), what
    assert np.array_equal(g_side, known.astype(np.uint8) | (unk.astype(np.uint8) << 1)), what
    kv, uv = kn_val[known].astype(np.float64), unk_val[unk].astype(np.float64)
    assert g_cnt.tolist() == [known.sum(), unk.sum(), np.isnan(kv).sum(), np.isnan(uv).sum(), bad.sum(), 0], what
    for k, v in ((0, kv), (2, uv)):
        v = v[~np.isnan(v)]
        if len(v):
            assert g_rng[k] == v.min() and g_rng[k + 1] == v.max(), (what, k)
        else:
            assert g_rng[k] == np.inf and g_rng[k + 1] == -np.inf, (what, k)


def labels_for(rng, N, C, with_unk2=True):
    gt = rng.integers(-2 if with_unk2 else -1, C, size=N)
    return gt.astype(np.int64)


SHAPES = [(1, 1, 1), (5, 2, 3), (300, 7, 5), (3001, 116, 116)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N,C,F", SHAPES)
def test_eval_values_score_metric(cuda, dtype, N, C, F):
    from openset_imagenet import _native as NV
    rng = np.random.default_rng(N * 131 + C)
    s = rng.random((N, C)).astype(dtype)
    if N >= 5:
        s[1, C - 1] = np.nan; s[2, 0] = np.inf; s[3, :] = -np.inf; s[4, 0] = np.nan
    for drop_last in (0, 1):
        Cc = C - drop_last
        if Cc < 1:                                           # np.amax over no column has no value: refused before any launch
            with pytest.raises(RuntimeError, match="code -1"):
                run_values(cuda, s, None, np.zeros(N, np.int64), NV.EVAL_SCORE, -1, drop_last)
            continue
        for unk_label, with_unk2 in ((-1, True), (-2, True), (-2, False), (3, True)):      # (-2, False): an empty side
            gt = labels_for(rng, N, C, with_unk2)
            if N >= 5:
                gt[0] = C + 2                                # beyond every column, never read
                gt[1] = Cc - 1; gt[2] = 0; gt[4] = -1 if unk_label == -1 else -2 if with_unk2 else -1
            bad = gt >= Cc
            known, unk = (gt >= 0) & ~bad, gt == unk_label
            kn_val = np.where(known, s[np.arange(N), np.where(known, gt, 0)], 0)           # 0 on rows without the known bit
            with np.errstate(invalid="ignore"):
                unk_val = s[:, :Cc].max(axis=1)
            got = run_values(cuda, s, None, gt, NV.EVAL_SCORE, unk_label, drop_last)
            check_values(got, kn_val, unk_val, known, unk, bad, (N, C, drop_last, unk_label, with_unk2))
            if unk_label == 3 and Cc > 3 and N >= 300:
                assert ((got[2] & 3) == 3).any()             # rows that are known and unknown at once
            if N >= 300 and drop_last:
                assert got[4][4] > 1


def float_midpoint_margin(n64, dtype):
    """Distance of each fp64 value from the nearest rounding midpoint of `dtype` (fp32), relative to the value."""
    a = n64.astype(dtype)
    b = np.nextafter(a, np.where(n64 >= a.astype(np.float64), dtype(np.inf), dtype(-np.inf)).astype(dtype))
    mid = (a.astype(np.float64) + b.astype(np.float64)) / 2
    return np.abs(n64 - mid) / n64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N,C,F", SHAPES)
def test_eval_values_norm_metric(cuda, dtype, N, C, F):
    """Norms against np.sqrt((f.astype(f64) ** 2).sum(1)).astype(T) on fixed-seed random features, equal bits.

    numpy sums pairwise, the device in index order; two fp64 summation orders differ by at most F * 2^-53 relative. float32: the
    test first ASSERTS that no row's fp64 norm lies within F * 2^-52 * norm of a rounding midpoint of float32, so both orders round
    to the same float. float64: a neighbouring double is never that far away, so the condition cannot be met by rounding room;
    the random features sit on a 2^-10 grid below 8 instead, where every square is a multiple of 2^-20 and every partial sum stays
    below 2^53 such units: the test asserts that, all summation orders then give the same double, and the one correctly rounded
    sqrt gives the same bits. Integer-valued features must agree without any condition."""
    from openset_imagenet import _native as NV
    rng = np.random.default_rng(N * 17 + F)
    if dtype == np.float32:
        f = rng.normal(size=(N, F)).astype(np.float32)
        n64 = np.sqrt((f.astype(np.float64) ** 2).sum(1))
        assert (float_midpoint_margin(n64, np.float32) > F * 2.0 ** -52).all()
    else:
        f = np.clip(np.round(rng.normal(size=(N, F)) * 1024) / 1024, -7.5, 7.5)
        assert np.array_equal(f * 1024, np.round(f * 1024)) and F * (np.abs(f).max() * 1024) ** 2 < 2.0 ** 53
    whole = rng.integers(-3, 4, size=(N, F)).astype(dtype)
    for feats, tag in ((f, "random"), (whole, "integers")):
        feats = feats.copy()
        if N >= 5:
            feats[1, F - 1] = np.nan; feats[2, 0] = np.inf; feats[3, :] = 0
        with np.errstate(invalid="ignore"):
            norm = host_norms(feats)
            if tag == "integers" and N >= 5:
                assert np.array_equal(norm[5:], np.linalg.norm(feats[5:], axis=1))         # the reference's own expression, same bits
        for unk_label, with_unk2 in ((-1, True), (-2, False), (3, True)):
            gt = labels_for(rng, N, C, with_unk2)
            if N >= 5:
                gt[0] = C + 2; gt[1] = 0; gt[2] = unk_label  # labels are not range-checked: C + 2 is a known row
            known, unk = gt >= 0, gt == unk_label
            got = run_values(cuda, None, feats, gt, NV.EVAL_NORM, unk_label, 0)
            check_values(got, norm, norm, known, unk, np.zeros(N, bool), (N, F, tag, unk_label, with_unk2))
            assert np.array_equal(got[0][known], norm[known], equal_nan=True)


# --------------------------------------------------------------------------------------------------- report, CCR at FPR
def synthetic_split(rng, N, C, dtype=np.float32):
    z = rng.normal(size=(N, C)) * 2
    s = np.exp(z - z.max(1, keepdims=True)); s = (s / s.sum(1, keepdims=True)).astype(dtype)
    gt = rng.integers(0, C - 1, size=N).astype(np.float32)   # get_arrays() returns the labels as fp32
    r = rng.random(N); gt[r < 0.2] = -1; gt[r > 0.75] = -2
    feats = rng.integers(-3, 4, size=(N, 9)).astype(dtype)
    return gt, s, feats


def test_ccr_at_fpr_is_oscr_then_the_rule(cuda):
    from openset_imagenet.util import calculate_oscr, ccr_at_fpr, nearest_fpr
    from oracle.oscr_oracle import calculate_oscr as oracle_oscr
    gt, s, _ = synthetic_split(np.random.default_rng(21), 2000, 8)
    for unk in (-1, -2):
        got = ccr_at_fpr(gt, s, unk_label=unk)
        assert got == nearest_fpr(*calculate_oscr(gt, s, unk_label=unk))
        ccr, fpr = oracle_oscr(gt, s, unk_label=unk)
        assert got == [fpr_rule(ccr, fpr, q) for q in (1e-3, 1e-2, 0.1, 1.0)]
        assert got[-1] is not None                           # the curve reaches fpr = 1 on this data
    assert ccr_at_fpr(gt, s, fpr_values=(0.5, 0.25), unk_label=-1, max_error=50.0) == \
        nearest_fpr(*calculate_oscr(gt, s, unk_label=-1), fpr_values=(0.5, 0.25), max_error=50.0)


@pytest.mark.parametrize("loss", ["entropic", "garbage"])
def test_evaluation_report_against_its_parts(cuda, loss):
    """Every entry of the report against numpy: np.histogram of the restated side values (30 bins), the restated FPR rule on the
    oracle's OSCR curve, and the confidences of metrics.py:8-42: the per-sample terms are float32 on both sides (scores[i, y] and
    1 + offset - max, formed in float32 as torch does), their sum runs in fp64 on the device in its own order: 400 terms below 2 are
    within 400 * 2 * 2^-53 < 1e-13 of any other fp64 order, bar 1e-12."""
    import json
    from openset_imagenet.script.evaluate import evaluation_report, table_row
    from oracle.oscr_oracle import calculate_oscr as oracle_oscr
    rng = np.random.default_rng(33)
    gt, s, feats = synthetic_split(rng, 400, 7)
    garbage = loss == "garbage"
    for present in ((-1, -2), (-1,)):
        y = gt if -2 in present else np.where(gt == -2, -1, gt)
        rep = evaluation_report(y, s, feats, loss)
        assert json.loads(json.dumps(rep)) == rep                                # plain values: what --report writes
        yi = y.astype(np.int64)
        known, unk2 = yi >= 0, yi == -2
        cols = s[:, :-1] if garbage else s
        offset = 0 if garbage else 1 / (yi.max() + 1)
        assert rep["conf_kn_count"] == known.sum() and rep["conf_unk_count"] == unk2.sum()
        assert abs(rep["conf_kn"] - s[known, yi[known]].astype(np.float64).sum() / known.sum()) <= 1e-12
        terms = (np.float32(1.0) + np.float32(offset)) - cols[unk2].max(1)      # float32 per sample, as torch and the kernel form it
        want_unk = terms.astype(np.float64).sum() / unk2.sum() if unk2.any() else 0.0
        assert abs(rep["conf_unk"] - want_unk) <= 1e-12
        assert sorted(rep["ccr_at_fpr"]) == sorted(rep["score_hist"]) == sorted(rep["norm_hist"]) == sorted(str(u) for u in present)
        for unk in present:
            ccr, fpr = oracle_oscr(yi, cols, unk_label=unk)
            assert rep["ccr_at_fpr"][str(unk)] == [fpr_rule(ccr, fpr, q) for q in rep["fpr_values"]]
            for key, metric in (("score_hist", "score"), ("norm_hist", "norm")):
                kn, un = side_values(s, feats, yi, unk, metric, garbage)
                want = np.histogram(kn, bins=30) + np.histogram(un, bins=30)
                for name, w in zip(("kn_hist", "kn_edges", "unk_hist", "unk_edges"), want):
                    assert rep[key][str(unk)][name] == w.tolist(), (loss, unk, key, name)
        row = table_row(rep, 2, loss, 57)
        cells = row.rstrip("\\").split(" & ")
        assert row.endswith("\\\\") and cells[0] == f"$P_2$ - {loss}" and cells[1] == "57" and len(cells) == 8
        assert cells[2:4] == [f"{rep['conf_kn']:1.3f}", f"{rep['conf_unk']:1.3f}"]
        want_cells = ["---" if v is None else f"{v:1.3f}" for v in rep["ccr_at_fpr"].get("-2", [None] * 4)]
        assert cells[4:] == want_cells

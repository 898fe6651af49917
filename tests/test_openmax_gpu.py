"""GPU parity of OpenMax (csrc/openmax.hip, openset_imagenet/openmax.py) against the fp64 numpy oracle of tests/openmax_oracle.py:
every stage through the C ABI on identical input bits, with 64-float guard bands around every output and a workspace full of 0xFF
bytes, then the whole of OpenMax.fit / predict, then the properties (same bits twice, row permutations, state dict, M = 1).

Bars. Counts, marks, shifts: exact. Means and distances: bit-exact on integer-valued inputs (the sums are exact), 1 fp32 ulp
otherwise. shape / scale: relative 1e-9 (the oracle's own reordering noise is <= 2e-15, fp32 resolution 6e-8). w-scores and
recalibrated probabilities: 1.2e-7 absolute, one fp32 ulp at 1 (both sides round an fp64 value once). End to end on integer-valued
features: 1e-6. End to end on real-valued features: E2E_REAL_BAR, see there."""
import numpy as np
import pytest
import torch

import openmax_oracle as O
from gpu_harness import Out, call, on, poisoned, same_bytes, ulps

pytestmark = pytest.mark.gpu

METRICS = (O.EUCLIDEAN, O.COSINE)
TAILS = (2, 20, 4096)

# Largest movement of the oracle's own probs when its fp32 distances (those of fit and those of predict) move by +-1 ulp at random,
# over E2E_CASES with five seeds each (openmax_oracle.jitter_movement; tests/test_openmax_cpu.py re-measures it): 2.7e-6.
# The bar is four times that.
E2E_MEASURED = 2.7e-6
E2E_REAL_BAR = 4 * E2E_MEASURED
E2E_TAIL, E2E_ALPHA = 20, 3
E2E_CASES = [(shape, metric) for shape in O.SHAPES for metric in METRICS]


# --------------------------------------------------------------------------------------------------------------- helpers
def workspace(N, C, F, cuda, fill=None):
    from openset_imagenet import _native as NL
    nb = NL.lib().osi_openmax_workspace(N, C, F)
    return poisoned(nb, cuda, fill), nb


def run_class_means(cuda, f, lg, gt, fill=None):
    from openset_imagenet import _native as NL
    (N, F), C = f.shape, lg.shape[1]
    df, dl, dg = on(cuda, f, lg, gt)
    ws, nb = workspace(N, C, F, cuda, fill)
    mav, count, correct = Out((C, F), torch.float32, cuda), Out((C,), torch.int64, cuda), Out((N,), torch.uint8, cuda)
    call(NL.lib().osi_openmax_class_means, df, dl, dg, N, C, F, mav, count, correct, ws, nb)
    assert mav.check() and count.check() and correct.check()
    return mav.np(), count.np(), correct.np()


def run_distances(cuda, f, mav, cls, metric):
    from openset_imagenet import _native as NL
    (N, F), C = f.shape, mav.shape[0]
    df, dm, dc = on(cuda, f, mav, cls)
    dist = Out((N,) if cls is not None else (N, C), torch.float32, cuda)
    call(NL.lib().osi_openmax_distances, df, dm, dc, N, C, F, metric, dist)
    assert dist.check()
    return dist.np()


def run_fit_tails(cuda, dist, gt, correct, C, T, fill=None):
    from openset_imagenet import _native as NL
    N = len(dist)
    dd, dg, dc = on(cuda, dist, gt, correct)
    ws, nb = workspace(N, C, 1, cuda, fill)
    outs = dict(shape=Out((C,), torch.float64, cuda), scale=Out((C,), torch.float64, cuda), shift=Out((C,), torch.float64, cuda),
                fitted=Out((C,), torch.uint8, cuda), tail_count=Out((C,), torch.int64, cuda), flags2=Out((2,), torch.int64, cuda))
    call(NL.lib().osi_openmax_fit_tails, dd, dg, dc, N, C, T, *outs.values(), ws, nb)
    assert all(o.check() for o in outs.values())
    return {k: o.np() for k, o in outs.items()}


def run_wscores(cuda, dist, shape, scale, shift, fitted):
    from openset_imagenet import _native as NL
    N, C = dist.shape
    w = Out((N, C), torch.float32, cuda)
    call(NL.lib().osi_openmax_wscores, *on(cuda, dist), N, C, *on(cuda, shape, scale, shift, fitted), w)
    assert w.check()
    return w.np()


def run_recalibrate(cuda, lg, w, alpha):
    from openset_imagenet import _native as NL
    N, C = lg.shape
    probs = Out((N, C + 1), torch.float32, cuda)
    call(NL.lib().osi_openmax_recalibrate, *on(cuda, lg, w), N, C, alpha, probs)
    assert probs.check()
    return probs.np()


def check_fit(got, want, where):
    for k in ("fitted", "tail_count", "flags2", "shift"):
        assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    for k in ("shape", "scale"):
        rel = np.abs(got[k] - want[k]) / np.where(want[k] != 0, np.abs(want[k]), 1.0)
        print(f"{where} {k}: max relative error {rel.max():.3e}")
        assert np.isfinite(got[k]).all() and rel.max() <= 1e-9, (where, k, got[k], want[k])


_CASES = {}


def case(shape, integer):
    """(features, logits, gt, oracle class means) of one shape: made once, shared, left unchanged."""
    key = (shape, integer)
    if key not in _CASES:
        f, lg, gt = O.make_case(*shape, seed=shape[0] + shape[2], integer=integer)
        _CASES[key] = (f, lg, gt, O.class_means(f, lg, gt))
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("shape", O.SHAPES)
@pytest.mark.parametrize("integer", (True, False))
def test_class_means(cuda, shape, integer):
    f, lg, gt, (mav_w, count_w, correct_w) = case(shape, integer)
    assert correct_w.sum() > 0 and (~correct_w).sum() > 0 and np.isnan(lg).any()
    mav, count, correct = run_class_means(cuda, f, lg, gt)
    assert np.array_equal(count, count_w) and np.array_equal(correct.astype(bool), correct_w)
    d = ulps(mav, mav_w)
    print(f"class_means {shape} integer={integer}: {d} ulp")
    assert d == 0 if integer else d <= 1


def test_class_means_without_a_correct_row_is_zero(cuda):
    f, lg, gt = (np.array(a) for a in case((97, 3, 1), True)[:3])
    gt[gt == 1] = -1                                     # class 1 loses every row
    mav, count, correct = run_class_means(cuda, f, lg, gt)
    mav_w, count_w, correct_w = O.class_means(f, lg, gt)
    assert count[1] == 0 and np.array_equal(count, count_w) and np.array_equal(correct.astype(bool), correct_w)
    assert same_bytes(mav, mav_w) and not mav[1].any()


@pytest.mark.parametrize("shape", O.SHAPES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("integer", (True, False))
def test_distances(cuda, shape, metric, integer):
    f, lg, gt, (mav, _, _) = case(shape, integer)
    if integer:
        mav = np.round(mav * 2).astype(np.float32)       # integer-valued means: every product and sum is exact
    for cls in (None, gt):
        want = O.distances(f, mav, cls, metric)
        got = run_distances(cuda, f, mav, cls, metric)
        d = ulps(got, want)
        print(f"distances {shape} metric={metric} integer={integer} cls={'all' if cls is None else 'own'}: {d} ulp")
        assert d == 0 if integer else d <= 1
    assert np.isnan(run_distances(cuda, f, mav, gt, metric)[(gt < 0) | (gt >= shape[1])]).all()


def test_cosine_zero_vector_is_nan(cuda):
    f = np.array([[0, 0, 0], [1, 2, 2]], dtype=np.float32)
    mav = np.array([[3, 0, 4], [0, 0, 0]], dtype=np.float32)
    got = run_distances(cuda, f, mav, None, O.COSINE)
    assert np.isnan(got[0]).all() and np.isnan(got[1, 1]) and got[1, 0] == np.float32(1 - 11 / 15)
    assert np.array_equal(got, O.distances(f, mav, None, O.COSINE), equal_nan=True)      # a NaN's sign and payload are not defined


@pytest.mark.parametrize("shape", O.SHAPES)
@pytest.mark.parametrize("T", TAILS)
def test_fit_tails(cuda, shape, T):
    N, C, _ = shape
    dist, gt, correct = O.make_tail_case(N, C, seed=N)
    want = O.fit_tails(dist, gt, correct, C, T)
    assert want["flags2"][0] == 2 and want["fitted"][0] == 1                       # the NaN and the +Inf of class 0 are left out
    if C >= 5:
        assert want["tail_count"][1] == 0 and want["tail_count"][2] == 1 and want["fitted"][3] == 0 and want["tail_count"][3] >= 2
    d0 = np.sort(dist[(gt == 0) & correct.astype(bool) & np.isfinite(dist)])        # ties across the tail boundary
    assert len(d0) > 21 and d0[-20] == d0[-21] and d0[-2] == d0[-3] and d0[-1] > d0[-2]
    check_fit(run_fit_tails(cuda, dist, gt, correct, C, T), want, f"fit_tails {shape} T={T}")


def test_fit_tails_negative_distances_and_collapsed_tail(cuda):
    """Cosine distances can be negative by a rounding, and a tail below 2^-53 collapses to x == 1 after the translation."""
    gt = np.zeros(40, dtype=np.int64); gt[20:] = 1
    correct = np.ones(40, dtype=np.uint8)
    rng = np.random.default_rng(4)
    dist = np.concatenate([rng.uniform(-0.5, 0.5, 20), [0.0, -0.0, 1e-30, 1e-20] * 5]).astype(np.float32)
    want = O.fit_tails(dist, gt, correct, 2, 10)
    assert want["fitted"].tolist() == [1, 0] and want["shift"][0] < 0.5
    check_fit(run_fit_tails(cuda, dist, gt, correct, 2, 10), want, "fit_tails negative / collapsed")


def test_wscores(cuda):
    rng = np.random.default_rng(11)
    N, C = 257, 5
    shape = np.array([1.5, 0.75, 0.0, 40.0, 3.0])
    scale = np.array([1.25, 2.0, 0.0, 1.5, 0.5])
    shift = np.array([3.0, 0.5, 0.0, 2.0, 7.0])
    fitted = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    dist = (8 * rng.random((N, C))).astype(np.float32)
    dist[::7, 0] = 2.0                                   # z = 0
    dist[1::7, 0] = 0.25                                 # z < 0
    dist[3, :] = np.nan
    dist[5, 1] = np.inf
    want = O.wscores(dist, shape, scale, shift, fitted)
    got = run_wscores(cuda, dist, shape, scale, shift, fitted)
    assert np.isnan(got[3]).all() and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    print(f"wscores: max abs error {np.abs(got[ok] - want[ok]).max():.3e}")
    assert np.abs(got[ok] - want[ok]).max() <= 1.2e-7
    keep = np.arange(N) != 3
    assert not got[keep, 2].any() and not got[::7, 0][np.arange(0, N, 7) != 3].any() and not got[1::7, 0].any()
    assert got[5, 1] == 1.0 and (got[ok] >= 0).all() and (got[ok] <= 1).all()


@pytest.mark.parametrize("shape", O.SHAPES)
def test_recalibrate(cuda, shape):
    N, C, _ = shape
    rng = np.random.default_rng(N)
    lg = rng.standard_normal((N, C)).astype(np.float32) * 3
    lg[1] = np.float32(0.5)                              # every logit tied
    lg[2] = -np.abs(lg[2]) - 1                           # all negative
    lg[4, : max(1, C // 2)] = lg[4].max() + 1            # a tie at the top
    lg[5, C - 1] = np.nan
    w = rng.random((N, C)).astype(np.float32)
    w[6] = 0
    w[7] = 1
    for alpha in (1, 3, C, C + 5):
        want = O.recalibrate(lg, w, alpha)
        got = run_recalibrate(cuda, lg, w, alpha)
        assert np.isnan(got[5]).all() and np.array_equal(np.isnan(got), np.isnan(want))
        ok = np.arange(N) != 5
        err, total = np.abs(got[ok] - want[ok]).max(), np.abs(got[ok].astype(np.float64).sum(1) - 1).max()
        print(f"recalibrate {shape} alpha={alpha}: max abs error {err:.3e}, rows sum to 1 within {total:.3e}")
        assert err <= 1.2e-7 and total <= 4e-7
        if alpha == C + 5:
            assert same_bytes(got, run_recalibrate(cuda, lg, w, C))


def test_recalibrate_tie_ranks_the_lower_index_first(cuda):
    lg = np.array([[1, 1, -2], [2, 4, 1]], dtype=np.float32)
    w = np.array([[1, 0.5, 0.5], [0.5, 0.25, 1]], dtype=np.float32)
    hat = np.array([[0, 0.75, -2, 1.25], [1.5, 3, 1, 1.5]])      # worked by hand in tests/test_openmax_cpu.py
    want = np.exp(hat) / np.exp(hat).sum(1, keepdims=True)
    assert np.abs(run_recalibrate(cuda, lg, w, 2) - want).max() <= 1.2e-7


# Sizes beyond the issue's shapes at which the kernels take another path: F above one workgroup's 256 columns (class means) and above
# several 32-column chunks (distances), C above one 64-class tile / one column per lane (distances, w-scores, recalibration), and tails
# that fill the 4096-key sort.
WIDE = (70, 130, 300)


def test_wide_features_and_many_classes(cuda):
    N, C, F = WIDE
    for integer in (True, False):
        f, lg, gt = O.make_case(N, C, F, seed=3, integer=integer)
        mav_w, count_w, correct_w = O.class_means(f, lg, gt)
        mav, count, correct = run_class_means(cuda, f, lg, gt)
        assert np.array_equal(count, count_w) and np.array_equal(correct.astype(bool), correct_w) and count.sum() > 20
        assert ulps(mav, mav_w) == 0 if integer else ulps(mav, mav_w) <= 1
        centres = np.round(mav_w * 2).astype(np.float32) if integer else mav_w
        for metric in METRICS:
            for cls in (None, gt):
                d = ulps(run_distances(cuda, f, centres, cls, metric), O.distances(f, centres, cls, metric))
                assert d == 0 if integer else d <= 1, (integer, metric, cls is None, d)
    rng = np.random.default_rng(8)
    dist = (8 * rng.random((N, C))).astype(np.float32)
    shape, scale, shift = 0.5 + 3 * rng.random(C), 0.5 + 2 * rng.random(C), 2 + 3 * rng.random(C)
    fitted = (rng.random(C) < 0.8).astype(np.uint8)
    w_want = O.wscores(dist, shape, scale, shift, fitted)
    w = run_wscores(cuda, dist, shape, scale, shift, fitted)
    assert np.abs(w - w_want).max() <= 1.2e-7 and not w[:, fitted == 0].any() and (w_want > 0).sum() > N
    lg = np.nan_to_num(lg, nan=0.0)
    lg[3, 60:70] = lg[3].max() + 1                       # a tie across the two halves of the columns a wave walks
    for alpha in (1, 3, C, C + 5):
        got, want = run_recalibrate(cuda, lg, w, alpha), O.recalibrate(lg, w, alpha)
        assert np.abs(got - want).max() <= 1.2e-7 and np.abs(got.astype(np.float64).sum(1) - 1).max() <= 4e-7, alpha


@pytest.mark.parametrize("T", (1000, 4096))
def test_fit_tails_that_fill_the_sort(cuda, T):
    """Two classes of about 4500 and 1500 eligible rows: tails of 1000 and 4096 are real selections (threshold inside the class), and
    4096 fills the LDS sort; the second class at T = 4096 takes every row it has. Quantised distances put ties on the boundary."""
    rng = np.random.default_rng(12)
    N = 6000
    gt = (rng.random(N) < 0.25).astype(np.int64)
    correct = np.ones(N, dtype=np.uint8)
    dist = (np.round((4 + rng.weibull(2.0, N)) * 512) / 512).astype(np.float32)
    want = O.fit_tails(dist, gt, correct, 2, T)
    assert want["tail_count"].tolist() == [T, min(T, int((gt == 1).sum()))] and want["fitted"].tolist() == [1, 1]
    d0 = np.sort(dist[gt == 0])
    assert d0[-T] == d0[-T - 1]
    check_fit(run_fit_tails(cuda, dist, gt, correct, 2, T), want, f"fit_tails N={N} T={T}")


# ------------------------------------------------------------------------------------------------------------ end to end
def fit_predict(shape, metric, integer, tailsize=E2E_TAIL, alpha=E2E_ALPHA, rows=None):
    from openset_imagenet.openmax import OpenMax
    f, lg, gt, _ = case(shape, integer)
    if rows is not None:
        f, lg, gt = f[rows], lg[rows], gt[rows]
    om = OpenMax(tailsize=tailsize, distance=("euclidean", "cosine")[metric], alpha=alpha).fit(f, lg, gt)
    return om, om.predict(lg, f)


@pytest.mark.parametrize("shape,metric", E2E_CASES)
def test_end_to_end_integer_features(cuda, shape, metric):
    f, lg, gt, _ = case(shape, True)
    om, probs = fit_predict(shape, metric, True)
    want = O.fit(f, lg, gt, E2E_TAIL, metric)
    assert probs.dtype == torch.float32 and probs.shape == (shape[0], shape[1] + 1) and probs.is_cuda
    assert same_bytes(om.mav.cpu().numpy(), want["mav"]) and np.array_equal(om.count.cpu().numpy(), want["count"])
    check_fit(dict(shape=om.shape.cpu().numpy(), scale=om.scale.cpu().numpy(), shift=om.shift.cpu().numpy(),
                   fitted=om.fitted.cpu().numpy(), tail_count=om.tail_count.cpu().numpy(), flags2=om.flags.cpu().numpy()),
              want, f"e2e integer {shape} metric={metric}")
    p, pw = probs.cpu().numpy(), O.predict(want, lg, f, E2E_ALPHA, metric)
    assert np.array_equal(np.isnan(p), np.isnan(pw))
    err = np.abs(p - pw)[~np.isnan(pw)].max(initial=0.0)        # F = 1 with the cosine distance: every row may be NaN
    print(f"e2e integer {shape} metric={metric}: max abs error {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("shape,metric", E2E_CASES)
def test_end_to_end_real_features(cuda, shape, metric):
    """Bar: the oracle's own probs move by up to 2.7e-6 (E2E_MEASURED) when its fp32 distances move by +-1 ulp at random (five
    seeds per case, these inputs); the bar is four times that, 1.08e-5 (E2E_REAL_BAR)."""
    f, lg, gt, _ = case(shape, False)
    om, probs = fit_predict(shape, metric, False)
    want = O.fit(f, lg, gt, E2E_TAIL, metric)
    assert np.array_equal(om.fitted.cpu().numpy(), want["fitted"]) and np.array_equal(om.count.cpu().numpy(), want["count"])
    p, pw = probs.cpu().numpy(), O.predict(want, lg, f, E2E_ALPHA, metric)
    assert np.array_equal(np.isnan(p), np.isnan(pw))
    err = np.nanmax(np.abs(p - pw))
    print(f"e2e real {shape} metric={metric}: max abs error {err:.3e} (bar {E2E_REAL_BAR:.3e})")
    assert err <= E2E_REAL_BAR
    w = om.w_scores(f).cpu().numpy()
    assert w.shape == (shape[0], shape[1]) and np.nanmin(w) >= 0 and np.nanmax(w) <= 1


# ------------------------------------------------------------------------------------------------------------ properties
def test_two_runs_give_identical_bits(cuda):
    shape = (600, 7, 33)
    for metric in METRICS:
        a, pa = fit_predict(shape, metric, False)
        b, pb = fit_predict(shape, metric, False)
        for name in ("mav", "shape", "scale", "shift", "fitted", "count", "tail_count", "flags"):
            assert same_bytes(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), (metric, name)
        assert same_bytes(pa.cpu().numpy(), pb.cpu().numpy())
        assert same_bytes(a.w_scores(case(shape, False)[0]).cpu().numpy(), b.w_scores(case(shape, False)[0]).cpu().numpy())


def test_row_permutation_leaves_the_fit_bit_identical(cuda):
    N, C = 600, 7
    dist, gt, correct = O.make_tail_case(N, C, seed=N)
    for T in TAILS:
        base = run_fit_tails(cuda, dist, gt, correct, C, T)
        for seed in range(3):
            p = np.random.default_rng(seed).permutation(N)
            again = run_fit_tails(cuda, dist[p], gt[p], correct[p], C, T)
            for k in ("shape", "scale", "shift", "fitted", "tail_count", "flags2"):
                assert same_bytes(base[k], again[k]), (T, seed, k)
    # through the class: integer-valued features, so the means (exact sums) and with them every distance keep their bits too
    shape = (300, 5, 130)
    a, _ = fit_predict(shape, O.EUCLIDEAN, True)
    b, _ = fit_predict(shape, O.EUCLIDEAN, True, rows=np.random.default_rng(5).permutation(shape[0]))
    for name in ("mav", "count", "shape", "scale", "shift", "fitted", "tail_count", "flags"):
        assert same_bytes(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), name


def test_workspace_contents_do_not_matter(cuda):
    f, lg, gt, _ = case((600, 7, 33), False)
    a, b = run_class_means(cuda, f, lg, gt, fill=None), run_class_means(cuda, f, lg, gt, fill=0)
    assert all(same_bytes(x, y) for x, y in zip(a, b))
    dist, gt2, correct = O.make_tail_case(600, 7, seed=600)
    a, b = run_fit_tails(cuda, dist, gt2, correct, 7, 20, fill=None), run_fit_tails(cuda, dist, gt2, correct, 7, 20, fill=0)
    assert all(same_bytes(a[k], b[k]) for k in a)


def test_predict_on_one_row_and_device_inputs(cuda):
    shape = (600, 7, 33)
    f, lg, gt, _ = case(shape, False)
    om, probs = fit_predict(shape, O.EUCLIDEAN, False)
    for i in (0, 17, 599):
        one = om.predict(lg[i:i + 1], f[i:i + 1])
        assert one.shape == (1, 8) and same_bytes(one.cpu().numpy(), probs[i:i + 1].cpu().numpy())
    dev = om.predict(torch.from_numpy(lg).to(cuda), torch.from_numpy(f).to(cuda))
    assert same_bytes(dev.cpu().numpy(), probs.cpu().numpy())
    assert om.predict(lg[:0], f[:0]).shape == (0, 8)
    assert np.array_equal(f, case(shape, False)[0])     # inputs are never written


def test_state_dict_gives_the_same_bits(cuda, tmp_path):
    from openset_imagenet.openmax import OpenMax
    shape = (300, 5, 130)
    f, lg, _, _ = case(shape, False)
    om, probs = fit_predict(shape, O.COSINE, False)
    sd = om.state_dict()
    assert all(not v.is_cuda for v in sd.values() if isinstance(v, torch.Tensor))
    torch.save(sd, tmp_path / "om.pth")
    again = OpenMax().load_state_dict(torch.load(tmp_path / "om.pth", weights_only=True))
    assert (again.tailsize, again.distance, again.alpha) == (E2E_TAIL, "cosine", E2E_ALPHA)
    assert same_bytes(again.predict(lg, f).cpu().numpy(), probs.cpu().numpy())


def test_torch_ops_match_the_abi(cuda):
    from openset_imagenet import _native as NL
    ops = NL.ops()
    f, lg, gt, _ = case((600, 7, 33), False)
    df, dl, dg = on(cuda, f, lg, gt)
    ws, _ = workspace(600, 7, 33, cuda)
    mav, count, correct = ops.openmax_class_means(df, dl, dg, ws)
    a = run_class_means(cuda, f, lg, gt)
    assert same_bytes(mav.cpu().numpy(), a[0]) and same_bytes(count.cpu().numpy(), a[1]) and same_bytes(correct.cpu().numpy(), a[2])
    dist = ops.openmax_distances(df, mav, dg, O.COSINE)
    assert same_bytes(dist.cpu().numpy(), run_distances(cuda, f, a[0], gt, O.COSINE))
    assert ops.openmax_distances(df, mav, None, O.EUCLIDEAN).shape == (600, 7)
    with pytest.raises(RuntimeError):
        ops.openmax_fit_tails(dist, dg, correct, 7, 1, ws)               # tailsize 1: refused by the ABI
    with pytest.raises(RuntimeError):
        ops.openmax_recalibrate(dl, dl[:, :3].contiguous(), 3)


def test_openmax_arrays_writes_the_five_keys(cuda, tmp_path):
    from openset_imagenet.script.evaluate import openmax_arrays
    from openset_imagenet import util
    f, lg, gt, _ = case((600, 7, 33), False)
    lg = np.nan_to_num(lg, nan=0.0)
    train = dict(gt=gt, logits=lg, features=f)
    split = dict(gt=gt[:97], logits=lg[:97], features=f[:97])
    om, arrays = openmax_arrays(train, split, 20, 3, "euclidean")
    assert sorted(arrays) == ["features", "gt", "logits", "scores", "unknown"]
    assert arrays["scores"].shape == (97, 7) and arrays["unknown"].shape == (97,) and arrays["scores"].dtype == np.float32
    assert all(isinstance(v, np.ndarray) for v in arrays.values())
    assert np.abs(arrays["scores"].astype(np.float64).sum(1) + arrays["unknown"] - 1).max() <= 4e-7
    want = O.predict(O.fit(f, lg, gt, 20, O.EUCLIDEAN), lg[:97], f[:97], 3, O.EUCLIDEAN)
    assert np.abs(arrays["scores"] - want[:, :7]).max() <= E2E_REAL_BAR and np.abs(arrays["unknown"] - want[:, 7]).max() <= E2E_REAL_BAR
    np.savez(tmp_path / "x_openmax.npz", **arrays)
    assert sorted(np.load(tmp_path / "x_openmax.npz").files) == sorted(arrays)
    _, again = openmax_arrays(om, split, 20, 3, "euclidean")             # a fitted object is taken as it is
    assert same_bytes(again["scores"], arrays["scores"])
    rows = arrays["gt"] < 7                                                # probs[:, :C] feeds the OSCR curve as it is
    ccr, fpr = util.calculate_oscr(arrays["gt"][rows], arrays["scores"][rows], unk_label=-1)
    assert len(ccr) == len(fpr) > 0

"""GPU parity of the Extreme Value Machine (csrc/evm.hip, openset_imagenet/evm.py) against the fp64 numpy oracle of
tests/evm_oracle.py: every stage through the C ABI on identical input bits, with 64-float guard bands around every output and a
workspace full of 0xFF bytes, then the whole of EVM.fit / predict, then the properties (same bits twice, column permutations, chunked
predict, state dict).

Bars. Distances on integer-valued features (|v| <= 4: dot products and norms are exact in fp32): bit-equal. Distances on real-valued
features: the project's matrix-core bound e = 2e-6 + 6e-8 sqrt(F) (tests/test_production_shapes_gpu.py) applied to |a||b|: cosine
|got - ref| <= e + 1.2e-7; Euclidean |got^2 - ref^2| <= 2 e |a||b| + 2.4e-7 ref^2. Tail fit: shifts, counts, marks and flags exact,
shape / scale relative 1e-9 (as tests/test_openmax_gpu.py). Cover: order and n_ev exact. Probabilities: 1.2e-7 absolute, one fp32 ulp
at 1 (both sides round an fp64 value once). End to end on real-valued features the oracle runs on the device's distances: the cover is
discrete, and a rounding-level change of a distance may legitimately flip a pick."""
import numpy as np
import pytest
import torch

import evm_oracle as E
from gpu_harness import Out, call, on, poisoned, same_bytes

pytestmark = pytest.mark.gpu

METRICS = (E.EUCLIDEAN, E.COSINE)
NAMES = {E.EUCLIDEAN: "euclidean", E.COSINE: "cosine"}
TAILS = (2, 20, 4096)
DIST_SHAPES = [(1, 1, 1), (3, 5, 3), (63, 127, 64), (65, 129, 130), (200, 70, 33), (129, 257, 2048)]
MULT = 0.5


# --------------------------------------------------------------------------------------------------------------- helpers
def workspace(R, N, F, cuda, fill=None):
    from openset_imagenet import _native as NL
    nb = NL.lib().osi_evm_workspace(R, N, F)
    return poisoned(nb, cuda, fill), nb


def run_distances(cuda, a, b, metric, fill=None, da=None):
    from openset_imagenet import _native as NL
    (R, F), N = a.shape, b.shape[0]
    ta, tb = on(cuda, a, b)
    ws, nb = workspace(R, N, F, cuda, fill)
    dist = Out((R, N), torch.float32, cuda)
    call(NL.lib().osi_evm_distances, ta if da is None else da, R, tb, N, F, metric, dist, ws, nb)
    assert dist.check()
    return dist.np()


def run_fit_rows(cuda, dist, N, gt, cls, T, fill=None):
    from openset_imagenet import _native as NL
    R, ld = dist.shape
    dd, dg = on(cuda, dist, gt)
    ws, nb = workspace(R, N, 1, cuda, fill)
    outs = dict(shape=Out((R,), torch.float64, cuda), scale=Out((R,), torch.float64, cuda), shift=Out((R,), torch.float64, cuda),
                fitted=Out((R,), torch.uint8, cuda), tail_count=Out((R,), torch.int64, cuda), flags2=Out((2,), torch.int64, cuda))
    call(NL.lib().osi_evm_fit_rows, dd, R, N, ld, dg, cls, T, MULT, *outs.values(), ws, nb)
    assert all(o.check() for o in outs.values())
    return {k: o.np() for k, o in outs.items()}


def run_set_cover(cuda, dpp, shape, scale, shift, fitted, threshold, fill=None):
    from openset_imagenet import _native as NL
    R = len(fitted)
    ws, nb = workspace(R, 1, 1, cuda, fill)
    order, n_ev = Out((R,), torch.int64, cuda), Out((1,), torch.int64, cuda)
    call(NL.lib().osi_evm_set_cover, *on(cuda, dpp), R, *on(cuda, shape, scale, shift, fitted), MULT, threshold, order, n_ev, ws, nb)
    assert order.check() and n_ev.check()
    return order.np(), int(n_ev.np()[0])


def run_probs(cuda, dist, V, shape, scale, shift, ev_start):
    from openset_imagenet import _native as NL
    M, ld = dist.shape
    C = len(ev_start) - 1
    probs = Out((M, C), torch.float32, cuda)
    call(NL.lib().osi_evm_probs, *on(cuda, dist), M, V, ld, *on(cuda, shape, scale, shift, ev_start), C, MULT, probs)
    assert probs.check()
    return probs.np()


def same_values(a, b):
    """Bit-equal where not NaN, NaN in the same places (a NaN's payload is not part of the definition)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(np.where(nan, np.float32(0), a).view(np.uint32), np.where(nan, np.float32(0), b).view(np.uint32))


def check_fit(got, want, where):
    for k in ("fitted", "tail_count", "flags2", "shift"):
        assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    for k in ("shape", "scale"):
        rel = np.abs(got[k] - want[k]) / np.where(want[k] != 0, np.abs(want[k]), 1.0)
        print(f"{where} {k}: max relative error {rel.max():.3e}")
        assert np.isfinite(got[k]).all() and rel.max() <= 1e-9, (where, k, got[k], want[k])


_PAIRS = {}


def pair(shape, integer):
    """(a [R, F], b [N, F]) of one shape: made once, shared, left unchanged."""
    key = (shape, integer)
    if key not in _PAIRS:
        R, N, F = shape
        _PAIRS[key] = (E.make_features(R, F, 11 * R + F, integer), E.make_features(N, F, 7 * N + F + 1, integer))
    return _PAIRS[key]


# ------------------------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", DIST_SHAPES)
def test_distances_integer_features_are_bit_equal(cuda, shape, metric):
    a, b = pair(shape, True)
    got = run_distances(cuda, a, b, metric)
    assert same_values(got, E.distances(a, b, metric)), (shape, metric)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", DIST_SHAPES)
def test_distances_real_features(cuda, shape, metric):
    a, b = pair(shape, False)
    got = run_distances(cuda, a, b, metric).astype(np.float64)
    ref = E.distances(a, b, metric).astype(np.float64)
    e = 2e-6 + 6e-8 * np.sqrt(shape[2])
    ab = np.sqrt(E.sq_norms(a))[:, None] * np.sqrt(E.sq_norms(b))[None, :]
    if metric == E.COSINE:
        err, bar = np.abs(got - ref), np.full_like(ref, e + 1.2e-7)
    else:
        err, bar = np.abs(got ** 2 - ref ** 2), 2 * e * ab + 2.4e-7 * ref ** 2
    print(f"{shape} {NAMES[metric]}: worst error / bar = {(err / bar).max():.3f}")
    assert np.isfinite(got).all() and (err <= bar).all(), (shape, metric, float((err / bar).max()))


def test_distances_take_the_same_bits_on_both_load_paths(cuda):
    """F % 4 == 0 and 16-byte aligned rows take 16-byte loads, anything else four 4-byte loads: `a` moved by one float."""
    a, b = pair((63, 127, 64), False)
    shifted = torch.zeros(a.size + 1, dtype=torch.float32, device=cuda)
    shifted[1:] = torch.from_numpy(a).to(cuda).reshape(-1)
    for metric in METRICS:
        assert same_bytes(run_distances(cuda, a, b, metric), run_distances(cuda, a, b, metric, da=shifted[1:]))


def test_distances_zero_nan_and_inf_rows(cuda):
    a, b = (x.copy() for x in pair((65, 129, 130), True))
    a[3] = 0                                                  # a zero row: NaN cosine against everything
    b[7] = 0
    a[10, 129], a[11, 0], a[64, 5] = np.nan, np.inf, -np.inf
    b[100, 64], b[128, 129], b[0, 0] = np.nan, np.inf, np.inf
    for metric in METRICS:
        got, want = run_distances(cuda, a, b, metric), E.distances(a, b, metric)
        assert same_values(got, want), metric
    cos = run_distances(cuda, a, b, E.COSINE)
    assert np.isnan(cos[3]).all() and np.isnan(cos[:, 7]).all() and np.isnan(cos[10]).all() and np.isnan(cos[:, 100]).all()
    assert np.isfinite(cos[20:60, 20:90]).all()             # the neighbours are untouched
    euc = run_distances(cuda, a, b, E.EUCLIDEAN)
    assert euc[3, 7] == 0 and np.isnan(euc[11, 0]) and np.isnan(euc[10]).all() and np.isfinite(euc[20:60, 20:90]).all()


# -------------------------------------------------------------------------------------------------------------- fit rows
FIT_N, FIT_C, FIT_CLS, FIT_PAD = 6000, 4, 1, 7
_FIT = {}


def fit_case(cuda):
    """(dist fp32 [12, N + 7], gt [N]): the DEVICE's Euclidean distances of 12 class-1 rows against 6000 rows (about 4700 negatives: the select of T = 4096 is a real one), then by row:
    0, 1 plain; 2 no candidate (every negative NaN); 3 one candidate; 4 ten candidates (fewer than T = 20); 5 a collapsed tail (all
    distances equal); 6 NaN, +Inf and -Inf among plain values; 7 quantised distances (ties, also across the tail's boundary) with -0
    and +0 among them; 8 .. 11 plain. The padding columns hold 0, the nearest possible value: a kernel that read them would choose
    them. Labels -1, -2, C and C + 2 are negatives like any other class."""
    if "case" not in _FIT:
        gt = E.make_labels(FIT_N, FIT_C, seed=5)
        b = E.make_features(FIT_N, 8, 21, False)
        a = b[np.flatnonzero(gt == FIT_CLS)[:12]]
        d = run_distances(cuda, a, b, E.EUCLIDEAN)
        neg = np.flatnonzero(gt != FIT_CLS)
        d[2, neg] = np.nan
        d[3, neg[1:]] = np.nan
        d[4, neg[10:]] = np.inf
        d[5, :] = np.float32(0.75)
        d[6, neg[::7]], d[6, neg[1::11]], d[6, neg[2::13]] = np.nan, np.inf, -np.inf
        d[7] = np.round(d[7] * 16) / 16
        d[7, neg[:3]], d[7, neg[3:5]] = np.float32(-0.0), np.float32(0.0)
        dist = np.zeros((12, FIT_N + FIT_PAD), dtype=np.float32)
        dist[:, :FIT_N] = d
        _FIT["case"] = (dist, gt)
    return _FIT["case"]


@pytest.mark.parametrize("T", TAILS)
def test_fit_rows(cuda, T):
    dist, gt = fit_case(cuda)
    got = run_fit_rows(cuda, dist, FIT_N, gt, FIT_CLS, T)
    want = E.fit_rows(dist, FIT_N, gt, FIT_CLS, T, MULT)
    check_fit(got, want, f"T={T}")
    assert got["tail_count"][[2, 3, 4]].tolist() == [0, 1, min(T, 10)] and got["fitted"][[2, 3, 5]].tolist() == [0, 0, 0]
    assert got["fitted"][[0, 1, 6, 8]].all() and got["fitted"][7] == (T > 5) and (got["shift"][got["fitted"] == 1] <= 0).all()
    assert (got["shape"][got["fitted"] == 0] == 0).all() and (got["scale"][got["fitted"] == 0] == 0).all()


def test_fit_rows_column_permutation_changes_no_bit(cuda):
    dist, gt = fit_case(cuda)
    for T in TAILS:
        base = run_fit_rows(cuda, dist, FIT_N, gt, FIT_CLS, T)
        for seed in range(2):
            p = np.random.default_rng(seed).permutation(FIT_N)
            again = run_fit_rows(cuda, np.ascontiguousarray(dist[:, :FIT_N][:, p]), FIT_N, gt[p], FIT_CLS, T)     # ld == N here
            for k in base:
                assert same_bytes(base[k], again[k]), (T, seed, k)


def test_fit_rows_labels_outside_the_classes_are_negatives(cuda):
    """cls = 0 of labels {0, -1, -2, C, C + 2}: every other row is a candidate; a class nobody carries sees all N."""
    dist, gt = fit_case(cuda)
    plain = np.ascontiguousarray(dist[[0, 1, 8, 9], :FIT_N])
    gt2 = np.where(gt == 0, 0, np.where(gt == 2, -1, np.where(gt == 3, -2, gt)))
    for cls in (0, 3, 77, -1):
        got = run_fit_rows(cuda, plain, FIT_N, gt2, cls, 20)
        check_fit(got, E.fit_rows(plain, FIT_N, gt2, cls, 20, MULT), f"cls={cls}")
    assert (run_fit_rows(cuda, plain, FIT_N, gt2, 77, 4096)["tail_count"] == 4096).all()


def test_fit_rows_workspace_contents_do_not_matter(cuda):
    dist, gt = fit_case(cuda)
    a, b = run_fit_rows(cuda, dist, FIT_N, gt, FIT_CLS, 20, fill=None), run_fit_rows(cuda, dist, FIT_N, gt, FIT_CLS, 20, fill=0)
    assert all(same_bytes(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------------- set cover
def cover_params(R, seed):
    """Points in the unit square, their Euclidean distances, and per-row Weibulls whose Psi runs from 0.99 (d = 0, small scale) down to
    0.05 (far away): never 1, so a threshold of 1 leaves nobody covered. About one row in nine is unfitted (all zeros)."""
    rng = np.random.default_rng(seed)
    x = rng.random((R, 2)).astype(np.float32)
    dpp = E.distances(x, x, E.EUCLIDEAN)
    fitted = (rng.random(R) > 0.11).astype(np.uint8)
    if R <= 2:
        fitted[:] = 1
    shape = np.where(fitted, 6.0, 0.0)
    scale = np.where(fitted, 1.0 + 0.4 * rng.random(R), 0.0)
    shift = np.where(fitted, -0.3, 0.0)                      # z = 0.5 (0.6 - d) + 1
    return dpp, shape, scale, shift, fitted


@pytest.mark.parametrize("R", (1, 2, 65, 300))
def test_set_cover(cuda, R):
    dpp, shape, scale, shift, fitted = cover_params(R, seed=R)
    n_fit = int(fitted.sum())
    for threshold, what in ((0.0, "one row covers all"), (1.0, "nobody covers anybody"), (0.5, "mixed"), (0.9, "mixed")):
        order, n = run_set_cover(cuda, dpp, shape, scale, shift, fitted, threshold)
        want, n_want = E.set_cover(dpp, shape, scale, shift, fitted, MULT, threshold)
        assert n == n_want and np.array_equal(order, want), (R, what, order[:10], want[:10])
        if threshold == 0.0:
            assert n == 1 and order[0] == np.flatnonzero(fitted)[0]
        if threshold == 1.0:
            assert n == n_fit and np.array_equal(order[:n], np.flatnonzero(fitted))
        assert (order[n:] == -1).all() and not (set(order[:n].tolist()) & set(np.flatnonzero(fitted == 0).tolist()))
    if R == 300:
        mixed = E.set_cover(dpp, shape, scale, shift, fitted, MULT, 0.5)[1]
        assert 1 < mixed < n_fit                             # the mixed case is one


@pytest.mark.parametrize("R", (2, 65, 300))
def test_set_cover_built_tie_and_unfitted_rows(cuda, R):
    """Distances of 0 (covered at any threshold below Psi(0)) or 10 (never covered). Row `p` covers the first half, row `q` the second:
    the same count, the lower index is picked first; row `m` covers the first half but one and is never needed. Unfitted rows sit in
    both halves, one of them with a row of zeros that would cover everything."""
    h = R // 2
    p, q, m = (0, 1, 0) if R == 2 else (5, h + 8, 20)
    dpp = np.full((R, R), 10, dtype=np.float32)
    np.fill_diagonal(dpp, 0)
    fitted = np.ones(R, dtype=np.uint8)
    if R > 2:
        dpp[p, :h], dpp[q, h:2 * h], dpp[m, :h - 1] = 0, 0, 0
        fitted[[7, h + 3]] = 0
        dpp[7, :] = 0
    shape, scale, shift = np.where(fitted, 2.0, 0.0), np.where(fitted, 1.0, 0.0), np.where(fitted, -0.5, 0.0)     # Psi(0) = 1 - exp(-2.25)
    order, n = run_set_cover(cuda, dpp, shape, scale, shift, fitted, 0.5)
    want, n_want = E.set_cover(dpp, shape, scale, shift, fitted, MULT, 0.5)
    assert n == n_want and np.array_equal(order, want), (order[:8], want[:8])
    if R == 2:
        assert order.tolist() == [0, 1]                      # each covers itself only: a tie at one
        fitted[0] = 0
        order, n = run_set_cover(cuda, dpp, np.array([0.0, 2.0]), np.array([0.0, 1.0]), np.array([0.0, -0.5]), fitted, 0.5)
        assert order.tolist() == [1, -1] and n == 1
        order, n = run_set_cover(cuda, dpp, np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2, dtype=np.uint8), 0.5)
        assert order.tolist() == [-1, -1] and n == 0
    else:
        assert order[:2].tolist() == [p, q] and n == 2 + (R - 2 * h) and 7 not in order and m not in order


def test_set_cover_workspace_contents_do_not_matter(cuda):
    args = cover_params(300, seed=300)
    a, b = run_set_cover(cuda, *args, 0.5, fill=None), run_set_cover(cuda, *args, 0.5, fill=0)
    assert same_bytes(a[0], b[0]) and a[1] == b[1]


# ----------------------------------------------------------------------------------------------------------------- probs
def test_probs(cuda):
    rng = np.random.default_rng(3)
    M, V, ld = 37, 9, 14
    dist = (2 * rng.random((M, ld))).astype(np.float32)
    dist[:, V:] = 0                                          # the padding would score highest
    dist[4, 1], dist[9, 8], dist[11, 5] = np.nan, np.nan, np.inf
    shape, scale, shift = 1 + 5 * rng.random(V), 0.5 + rng.random(V), -0.5 - rng.random(V)
    ev_start = np.array([0, 3, 3, 8, 9], dtype=np.int64)     # class 1 has no extreme vector, class 3 one
    got, want = run_probs(cuda, dist, V, shape, scale, shift, ev_start), E.probs(dist, V, shape, scale, shift, ev_start, MULT)
    assert got.shape == (M, 4) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[4, 0]) and np.isnan(got[9, 3]) and np.isnan(got).sum() == 2 and (got[:, 1] == 0).all()
    err = np.nanmax(np.abs(got.astype(np.float64) - want))
    print(f"probs: max error {err:.3e}")
    assert err <= 1.2e-7 and np.nanmin(got) >= 0 and np.nanmax(got) <= 1 and 0 < np.nanmax(got[:, 0])
    # V = 1, and an entry with scale 0 counts as unfitted
    one = run_probs(cuda, dist[:, :1].copy(), 1, shape[:1], scale[:1], shift[:1], np.array([0, 1], dtype=np.int64))
    assert np.nanmax(np.abs(one[:, 0].astype(np.float64) - E.probs(dist[:, :1], 1, shape[:1], scale[:1], shift[:1], [0, 1], MULT)[:, 0])) <= 1.2e-7
    dead = run_probs(cuda, dist[:3, :1].copy(), 1, np.zeros(1), np.zeros(1), np.zeros(1), np.array([0, 1], dtype=np.int64))
    assert (dead == 0).all()


# ------------------------------------------------------------------------------------------------------------ end to end
E2E_TAIL = 20
E2E_INT = [((300, 5, 16), E.COSINE), ((300, 5, 16), E.EUCLIDEAN), ((97, 3, 1), E.EUCLIDEAN), ((97, 3, 1), E.COSINE)]
_E2E = {}


def e2e_case(shape, integer):
    key = (shape, integer)
    if key not in _E2E:
        _E2E[key] = E.make_case(*shape, seed=shape[0] + shape[2], integer=integer)
    return _E2E[key]


def fit_device(shape, integer, metric, cover, **kw):
    from openset_imagenet.evm import EVM
    f, gt = e2e_case(shape, integer)
    return EVM(tailsize=E2E_TAIL, cover_threshold=cover, distance_multiplier=MULT, distance=NAMES[metric], **kw).fit(f, gt)


def check_model(evm, want, where):
    host = {k: getattr(evm, k).cpu().numpy() for k in ("ev_features", "ev_shape", "ev_scale", "ev_shift", "ev_start", "flags")}
    assert np.array_equal(host["ev_start"], want["ev_start"]), (where, host["ev_start"], want["ev_start"])
    assert same_bytes(host["ev_features"], want["ev_features"]), where       # the same rows in the same order
    assert np.array_equal(host["ev_shift"], want["ev_shift"]) and np.array_equal(host["flags"], want["flags"]), where
    for k in ("ev_shape", "ev_scale"):
        if len(want[k]):
            rel = np.abs(host[k] - want[k]) / np.abs(want[k])
            assert rel.max() <= 1e-9, (where, k, rel.max())


@pytest.mark.parametrize("cover", (None, 0.5))
@pytest.mark.parametrize("shape,metric", E2E_INT)
def test_end_to_end_integer_features(cuda, shape, metric, cover):
    f, gt = e2e_case(shape, True)
    evm = fit_device(shape, True, metric, cover)
    want = E.fit(f, gt, E2E_TAIL, MULT, metric, threshold=cover)
    check_model(evm, want, (shape, metric, cover))
    q = E.make_features(61, shape[2], 99, True)
    got, ref = evm.predict(q).cpu().numpy(), E.predict(want, q, MULT, metric)
    assert got.shape == (61, shape[1]) and got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(ref))
    err = np.nanmax(np.abs(got.astype(np.float64) - ref)) if np.isfinite(ref).any() else 0.0
    print(f"{shape} {NAMES[metric]} cover {cover}: {len(want['ev_shape'])} extreme vectors, max error {err:.3e}")
    assert err <= 1.2e-7


@pytest.mark.parametrize("cover", (None, 0.5))
@pytest.mark.parametrize("metric", METRICS)
def test_end_to_end_real_features_on_the_device_s_distances(cuda, metric, cover):
    from openset_imagenet import _native as NL
    shape = (300, 5, 16)
    f, gt = e2e_case(shape, False)

    def device_distances(a, b):
        ta, tb = on(cuda, a, b)
        ws, _ = workspace(len(a), len(b), a.shape[1], cuda)
        return NL.ops().evm_distances(ta, tb, metric, ws).cpu().numpy()

    evm = fit_device(shape, False, metric, cover)
    want = E.fit(f, gt, E2E_TAIL, MULT, metric, threshold=cover, dist_fn=device_distances)
    check_model(evm, want, (metric, cover))
    assert 0 < len(want["ev_shape"]) and (np.diff(want["ev_start"]) > 0).all()
    q = E.make_case(83, 5, 16, seed=316, integer=False)[0]
    got, ref = evm.predict(q).cpu().numpy(), E.predict(want, q, MULT, metric, dist_fn=device_distances)
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"{NAMES[metric]} cover {cover}: {len(want['ev_shape'])} extreme vectors, max error {err:.3e}")
    assert err <= 1.2e-7 and got.max() > 0.5
    if cover is not None:
        assert len(want["ev_shape"]) < int((gt >= 0).sum())                                 # the cover reduces the model


def test_use_negatives_false_drops_the_negative_rows(cuda):
    shape = (300, 5, 16)
    f, gt = e2e_case(shape, True)
    evm = fit_device(shape, True, E.EUCLIDEAN, None, use_negatives=False)
    check_model(evm, E.fit(f, gt, E2E_TAIL, MULT, E.EUCLIDEAN, use_negatives=False), "use_negatives=False")
    both = fit_device(shape, True, E.EUCLIDEAN, None)
    assert not same_bytes(evm.ev_shift.cpu().numpy(), both.ev_shift.cpu().numpy())      # the negatives were among the nearest


# ------------------------------------------------------------------------------------------------------------ properties
def test_two_runs_give_identical_bits(cuda):
    shape = (300, 5, 16)
    q = e2e_case(shape, False)[0][:50]
    for metric in METRICS:
        a, b = fit_device(shape, False, metric, 0.5), fit_device(shape, False, metric, 0.5)
        for name in ("ev_features", "ev_shape", "ev_scale", "ev_shift", "ev_start", "flags"):
            assert same_bytes(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), (metric, name)
        assert same_bytes(a.predict(q).cpu().numpy(), b.predict(q).cpu().numpy())


def test_chunked_predict_and_device_inputs(cuda):
    shape = (300, 5, 16)
    f, gt = e2e_case(shape, False)
    evm = fit_device(shape, False, E.COSINE, None)
    whole = evm.predict(f).cpu().numpy()
    for chunk in (1, 7, 128, 299, 1000):
        assert same_bytes(evm.predict(f, chunk=chunk).cpu().numpy(), whole), chunk
    assert same_bytes(evm.predict(torch.from_numpy(f).to(cuda)).cpu().numpy(), whole)
    assert same_bytes(evm.predict(f[17:18]).cpu().numpy(), whole[17:18]) and evm.predict(f[:0]).shape == (0, 5)
    assert np.array_equal(f, e2e_case(shape, False)[0])     # inputs are never written
    dev_fit = fit_device(shape, False, E.COSINE, None)
    dev_fit.fit(torch.from_numpy(f).to(cuda), torch.from_numpy(gt).to(cuda))
    assert same_bytes(dev_fit.ev_shape.cpu().numpy(), evm.ev_shape.cpu().numpy())


def test_state_dict_gives_the_same_bits(cuda, tmp_path):
    from openset_imagenet.evm import EVM
    shape = (300, 5, 16)
    f, _ = e2e_case(shape, False)
    evm = fit_device(shape, False, E.EUCLIDEAN, 0.5)
    sd = evm.state_dict()
    assert all(not v.is_cuda for v in sd.values() if isinstance(v, torch.Tensor))
    torch.save(sd, tmp_path / "evm.pth")
    again = EVM().load_state_dict(torch.load(tmp_path / "evm.pth", weights_only=True))
    assert (again.tailsize, again.cover_threshold, again.distance, again.distance_multiplier) == (E2E_TAIL, 0.5, "euclidean", MULT)
    assert not again.ev_features.is_cuda                    # the state moves on first use
    assert same_bytes(again.predict(f).cpu().numpy(), evm.predict(f).cpu().numpy()) and again.ev_features.is_cuda


def test_torch_ops_match_the_abi(cuda):
    from openset_imagenet import _native as NL
    ops = NL.ops()
    dist, gt = fit_case(cuda)
    a, b = pair((65, 129, 130), False)
    ta, tb = on(cuda, a, b)
    ws, _ = workspace(65, 129, 130, cuda)
    assert same_bytes(ops.evm_distances(ta, tb, E.COSINE, ws).cpu().numpy(), run_distances(cuda, a, b, E.COSINE))
    big_ws, _ = workspace(300, FIT_N, 1, cuda)
    out = ops.evm_fit_rows(*on(cuda, dist, gt), FIT_CLS, 20, MULT, big_ws)
    ref = run_fit_rows(cuda, dist, FIT_N, gt, FIT_CLS, 20)
    for got, k in zip(out, ("shape", "scale", "shift", "fitted", "tail_count", "flags2")):
        assert same_bytes(got.cpu().numpy(), ref[k]), k
    args = cover_params(300, seed=300)
    order, n_ev = ops.evm_set_cover(*on(cuda, *args), MULT, 0.5, big_ws)
    ref_order, ref_n = run_set_cover(cuda, *args, 0.5)
    assert same_bytes(order.cpu().numpy(), ref_order) and int(n_ev) == ref_n
    rng = np.random.default_rng(8)
    d, shape, scale, shift = (2 * rng.random((20, 6))).astype(np.float32), 1 + rng.random(6), 1 + rng.random(6), -rng.random(6)
    start = np.array([0, 2, 6], dtype=np.int64)
    assert same_bytes(ops.evm_probs(*on(cuda, d, shape, scale, shift, start), MULT).cpu().numpy(),
                     run_probs(cuda, d, 6, shape, scale, shift, start))
    with pytest.raises(RuntimeError):
        ops.evm_fit_rows(*on(cuda, dist, gt), FIT_CLS, 1, MULT, big_ws)                # tailsize 1: refused by the ABI
    with pytest.raises(RuntimeError):
        ops.evm_distances(ta, tb[:, :100].contiguous(), E.COSINE, ws)


def test_evm_arrays_writes_its_keys(cuda, tmp_path):
    from openset_imagenet.script.evaluate import evm_arrays
    from openset_imagenet import util
    f, gt = e2e_case((300, 5, 16), True)              # unclustered: the scores of the known rows do not all saturate at 1
    logits = f[:, :5].copy()
    train = dict(gt=gt, logits=logits, features=f)
    split = dict(gt=gt[:97], logits=logits[:97], features=f[:97])
    evm, arrays = evm_arrays(train, split, E2E_TAIL, cover_threshold=0.5, multiplier=MULT, distance="cosine")
    assert sorted(arrays) == ["features", "gt", "logits", "scores"]
    assert arrays["scores"].shape == (97, 5) and arrays["scores"].dtype == np.float32
    assert all(isinstance(v, np.ndarray) for v in arrays.values())
    assert same_bytes(arrays["scores"], fit_device((300, 5, 16), True, E.COSINE, 0.5).predict(f[:97]).cpu().numpy())
    np.savez(tmp_path / "x_evm.npz", **arrays)
    assert sorted(np.load(tmp_path / "x_evm.npz").files) == sorted(arrays)
    _, again = evm_arrays(evm, split, E2E_TAIL)              # a fitted object is taken as it is
    assert same_bytes(again["scores"], arrays["scores"])
    rows = arrays["gt"] != -2                                # the scores feed the OSCR curve as they are
    ccr, fpr = util.calculate_oscr(arrays["gt"][rows], arrays["scores"][rows], unk_label=-1)
    assert len(ccr) == len(fpr) > 0

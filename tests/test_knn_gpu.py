"""GPU parity of deep nearest neighbours (csrc/knn.hip, openset_imagenet/knn.py) against the numpy oracle of tests/knn_oracle.py: both
kernels through the C ABI on identical input bits, with 256-byte guard bands around every output, a workspace full of 0xFF bytes and
ld > N with padding columns of -Inf that must never be selected, then the whole of KNN.fit / predict / unknown_score / kneighbors /
calibrate, then the properties (same bits twice, C = 1 against topk, permuted segments, strict index order on ties, chunked predict,
state dict).

The bar is EXACT EQUALITY everywhere, NaN positions equal: selection does no arithmetic, and the three transforms are single fp32
operations the oracle repeats in np.float32. End to end the oracle runs on the device's own distance bits, read back from
evm_distances: a rounding-level difference in a distance may then not flip a rank (the rule of tests/test_evm_gpu.py)."""
import numpy as np
import pytest
import torch

import evm_oracle as E
import knn_oracle as K
from gpu_harness import Out, call, on, poisoned

pytestmark = pytest.mark.gpu

PAD = 3                                      # padding columns behind the N used ones
KS = (1, 2, 64, 1024)
NS = (1, 63, 64, 65, 257, 4097)              # around the wave, more than one tile of 2048 columns (and than one wave's 2048)
KINDS = ("integer", "real", "salted")
TRANSFORMS = (K.RAW, K.SIM_COSINE, K.SIM_INVERSE)


# --------------------------------------------------------------------------------------------------------------- helpers
def workspace(M, N, k, cuda):
    from openset_imagenet import _native as NL
    nb = NL.lib().osi_knn_workspace(M, N, k)
    return poisoned(nb, cuda), nb


def run_topk(cuda, dist, N, k, skip=None):
    from openset_imagenet import _native as NL
    M, ld = dist.shape
    ws, nb = workspace(M, N, k, cuda)
    d, i = Out((M, k), torch.float32, cuda), Out((M, k), torch.int64, cuda)
    call(NL.lib().osi_knn_topk, *on(cuda, dist), M, N, ld, k, *on(cuda, skip), d, i, ws, nb)
    assert d.check() and i.check()
    return d.np(), i.np()


def run_class_kth(cuda, dist, N, start, k, skip=None, what=K.RAW):
    from openset_imagenet import _native as NL
    M, ld = dist.shape
    C = len(start) - 1
    ws, nb = workspace(M, N, k, cuda)
    out = Out((M, C), torch.float32, cuda)
    call(NL.lib().osi_knn_class_kth, *on(cuda, dist), M, N, ld, *on(cuda, np.asarray(start, dtype=np.int64)), C, k, *on(cuda, skip), what,
         out, ws, nb)
    assert out.check()
    return out.np()


_MATRICES = {}


def matrix(kind, M, N):
    """dist [M, N + PAD] fp32 of one kind and shape: made once, shared, left unchanged. Padding columns hold -Inf. integer: values
    0 .. 3, ties are the rule. salted: real values with NaN, +Inf, -Inf, -0 and +0 strewn in; row 1 is all NaN, row 2 is NaN but
    for its first column (its k-th element is a NaN for every k >= 2), row 3 holds -0 and +0 only."""
    key = (kind, M, N)
    if key not in _MATRICES:
        rng = np.random.default_rng(1000 * N + 10 * M + len(kind))
        if kind == "integer":
            d = rng.integers(0, 4, (M, N)).astype(np.float32)
        else:
            d = (rng.standard_normal((M, N)) * 3).astype(np.float32)
        if kind == "salted":
            salt = rng.random((M, N))
            for lo, v in ((0.00, np.nan), (0.04, np.inf), (0.08, -np.inf), (0.12, -0.0), (0.16, 0.0)):
                d[(salt >= lo) & (salt < lo + 0.04)] = v
            d[3::4] = np.round(d[3::4])                   # rows with ties among real values
            if M > 1:
                d[1] = np.nan
            if M > 2:
                d[2, 1:] = np.nan
            if M > 3:
                d[3] = np.where(rng.random(N) < 0.5, np.float32(-0.0), np.float32(0.0))
        full = np.full((M, N + PAD), -np.inf, dtype=np.float32)
        full[:, :N] = d
        full.setflags(write=False)
        _MATRICES[key] = full
    return _MATRICES[key]


def own_minimum(dist, N):
    """Per row the column the order ranks first."""
    return K.topk(dist, N, 1)[1][:, 0].copy()


def skips(dist, N):
    M = len(dist)
    return (None, np.full(M, -1, dtype=np.int64), np.full(M, N, dtype=np.int64), own_minimum(dist, N))


def check_topk(cuda, dist, N, k, skip, where):
    d, i = run_topk(cuda, dist, N, k, skip)
    want_d, want_i = K.topk(dist, N, k, skip)
    assert np.array_equal(i, want_i), (where, i, want_i)
    assert K.same_values(d, want_d), (where, d, want_d)
    return d, i


# ------------------------------------------------------------------------------------------------------------------ topk
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", NS)
def test_topk_equals_the_oracle(cuda, N, kind):
    """K = 1, 2, 64, 1024 (K > N included) under every skip: NULL, -1, N, the row's own minimum."""
    dist = matrix(kind, 5, N)
    for k in KS:
        for s, skip in enumerate(skips(dist, N)):
            d, i = check_topk(cuda, dist, N, k, skip, (kind, N, k, s))
            assert (i < N).all()                          # never a padding column
            if s == 3:
                assert (i != skip[:, None]).all()


@pytest.mark.parametrize("kind", ("integer", "real"))
def test_topk_of_long_rows(cuda, kind):
    """N = 70 000, M = 3: thirty-five tiles, the buffer is cut back many times."""
    dist = matrix(kind, 3, 70000)
    for k in (1, 64, 1024):
        check_topk(cuda, dist, 70000, k, None, (kind, k))
    check_topk(cuda, dist, 70000, 64, own_minimum(dist, 70000), (kind, "skip"))


def test_topk_indices_are_strictly_ordered_on_ties_and_calls_repeat(cuda):
    dist = matrix("integer", 5, 4097)
    d, i = run_topk(cuda, dist, 4097, 1024)
    assert (np.diff(d, axis=1) >= 0).all()
    assert (np.diff(i, axis=1)[np.diff(d, axis=1) == 0] > 0).all()
    d2, i2 = run_topk(cuda, dist, 4097, 1024)
    assert d.tobytes() == d2.tobytes() and i.tobytes() == i2.tobytes()


# ------------------------------------------------------------------------------------------------------------- class_kth
def segments(N, k):
    """start [C + 1] over N columns: a first value below 0 (an empty first class once clamped), classes of length 1, k - 1, k, k + 1,
    boundaries at 63 / 64 / 65, an empty middle class, a descending pair, the rest, and an empty last class ending beyond N."""
    cuts = [-7, 0]
    for length in (1, k - 1, k, k + 1):
        cuts.append(cuts[-1] + length)
    cuts += [c for c in (63, 64, 65) if c > cuts[-1]]
    cuts += [cuts[-1], 40, 70]                            # an empty class, a descending pair, a class that starts again at 40
    cuts += [max(70, N // 2), N, N + 9]
    return np.array(cuts, dtype=np.int64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", NS)
def test_class_kth_equals_the_oracle(cuda, N, kind):
    dist = matrix(kind, 5, N)
    for k in KS:
        start = segments(N, k)
        for s, skip in enumerate(skips(dist, N)):
            for what in (TRANSFORMS if (k == 2 or s == 0) else (K.RAW,)):
                got = run_class_kth(cuda, dist, N, start, k, skip, what)
                want = K.class_kth(dist, N, start, k, skip, what)
                assert K.same_values(got, want), (kind, N, k, s, what, got, want)


def test_class_kth_skipping_the_only_column_of_a_class(cuda):
    dist = matrix("real", 5, 257)
    start = np.array([0, 1, 2, 257])
    for what in TRANSFORMS:
        got = run_class_kth(cuda, dist, 257, start, 1, np.array([0, 1, 0, 1, 5], dtype=np.int64), what)
        empty = np.float32(np.inf) if what == K.RAW else np.float32(0)
        assert got[0, 0] == got[2, 0] == got[1, 1] == got[3, 1] == empty and np.isfinite(got[4]).all()
        assert K.same_values(got, K.class_kth(dist, 257, start, 1, np.array([0, 1, 0, 1, 5]), what))


@pytest.mark.parametrize("kind", ("integer", "real"))
def test_class_kth_one_long_class_beside_one_column_classes(cuda, kind):
    """A 60 000-column class (far above any staging size) between one-column classes, N = 70 000, M = 3."""
    dist = matrix(kind, 3, 70000)
    start = np.array([0, 1, 2, 60002, 60003, 70000])
    for k in (1, 64, 1024):
        got = run_class_kth(cuda, dist, 70000, start, k)
        assert K.same_values(got, K.class_kth(dist, 70000, start, k)), (kind, k)
    skip = own_minimum(dist, 70000)
    assert K.same_values(run_class_kth(cuda, dist, 70000, start, 64, skip, K.SIM_INVERSE),
                         K.class_kth(dist, 70000, start, 64, skip, K.SIM_INVERSE))


@pytest.mark.parametrize("kind", KINDS)
def test_class_kth_around_the_one_wave_length(cuda, kind):
    """Segments of up to 2048 columns are one wave's work, longer ones a workgroup's: lengths 2047, 2048, 2049 side by side, then a
    segment of exactly one tile more."""
    dist = matrix(kind, 3, 70000)
    start = np.array([0, 2047, 4095, 6144, 6144 + 4096, 6144 + 4096 + 2048, 70000])
    skip = np.array([2046, 4094, 6143], dtype=np.int64)  # the last column of the first three segments, one per row
    for k in KS:
        for sk in (None, skip):
            got = run_class_kth(cuda, dist, 70000, start, k, sk, K.SIM_INVERSE)
            assert K.same_values(got, K.class_kth(dist, 70000, start, k, sk, K.SIM_INVERSE)), (kind, k)


@pytest.mark.parametrize("kind", KINDS)
def test_class_kth_of_one_class_is_a_column_of_topk(cuda, kind):
    for N in (65, 4097):
        dist = matrix(kind, 5, N)
        for k in KS:
            for skip in (None, own_minimum(dist, N)):
                kth = run_class_kth(cuda, dist, N, np.array([0, N]), k, skip)
                d, _ = run_topk(cuda, dist, N, k, skip)
                n = N - (0 if skip is None else 1)
                assert K.same_values(kth[:, 0], d[:, min(k, n) - 1]), (kind, N, k)
                again = run_class_kth(cuda, dist, N, np.array([0, N]), k, skip)
                assert kth.tobytes() == again.tobytes()


def test_class_kth_permuting_segments_permutes_columns(cuda):
    N, k = 4097, 64
    dist = matrix("salted", 5, N)
    bounds = np.array([0, 1, 64, 129, 129, 2300, 4097])
    base = run_class_kth(cuda, dist, N, bounds, k, None, K.SIM_COSINE)
    perm = np.array([4, 0, 5, 2, 3, 1])
    pieces = [dist[:, bounds[c]:bounds[c + 1]] for c in perm]
    moved = np.full_like(dist, -np.inf)
    moved[:, :N] = np.concatenate(pieces, axis=1)
    start = np.concatenate([[0], np.cumsum([p.shape[1] for p in pieces])])
    got = run_class_kth(cuda, moved, N, start, k, None, K.SIM_COSINE)
    assert K.same_values(got, base[:, perm])


# ------------------------------------------------------------------------------------------------------------ end to end
E2E = {"small": (50, 200, 64, 6), "wide": (129, 257, 2048, 7)}       # M queries, N training rows, F, classes (one of them empty)
_E2E = {}


def e2e_case(name):
    if name not in _E2E:
        M, N, F, C = E2E[name]
        train, query = E.make_features(N, F, 5 * N + F, False), E.make_features(M, F, 3 * M + F, False)
        rng = np.random.default_rng(N + F)
        gt = rng.integers(0, C - 1, N)
        gt[gt == 2] = C - 1                               # class 2 has no rows
        gt[rng.random(N) < 0.1] = -1
        _E2E[name] = (train, gt.astype(np.int64), query)
    return _E2E[name]


def device_distances(knn, q, cuda):
    from openset_imagenet import _native as NL
    q = torch.as_tensor(q).to(cuda).float().contiguous()
    ws = torch.empty(NL.lib().osi_evm_workspace(q.shape[0], knn.bank_features.shape[0], q.shape[1]), dtype=torch.uint8, device=cuda)
    metric = E.COSINE if knn.distance == "cosine" else E.EUCLIDEAN
    return NL.ops().evm_distances(q, knn.bank_features, metric, ws).cpu().numpy()


@pytest.mark.parametrize("distance", ("cosine", "euclidean"))
@pytest.mark.parametrize("name", sorted(E2E))
def test_knn_end_to_end(cuda, name, distance):
    from openset_imagenet.knn import KNN, bank_selection
    train, gt, query = e2e_case(name)
    k = 5
    knn = KNN(k=k, distance=distance).fit(train, gt)
    rows, start = bank_selection(gt)
    n = len(rows)
    assert knn.bank_rows.cpu().numpy().tolist() == rows.tolist() and knn.bank_start.cpu().numpy().tolist() == start.tolist()
    assert np.array_equal(knn.bank_features.cpu().numpy(), train[rows]) and np.array_equal(knn.bank_labels.cpu().numpy(), gt[rows])
    dist = device_distances(knn, query, cuda)
    what = K.SIM_COSINE if distance == "cosine" else K.SIM_INVERSE
    scores = knn.predict(query)
    assert scores.is_cuda and scores.dtype == torch.float32
    assert K.same_values(scores.cpu().numpy(), K.class_kth(dist, n, start, k, None, what))
    assert (scores[:, 2] == 0).all() and bool(((scores >= 0) & (scores <= 1)).all())
    assert K.same_values(knn.unknown_score(query).cpu().numpy(), K.class_kth(dist, n, [0, n], k)[:, 0])
    d, idx = knn.kneighbors(query)
    want_d, want_i = K.topk(dist, n, k)
    assert K.same_values(d.cpu().numpy(), want_d) and np.array_equal(idx.cpu().numpy(), rows[want_i])
    # chunked equals unchunked
    assert torch.equal(knn.predict(query, chunk=7), scores) and torch.equal(knn.unknown_score(query, chunk=7), knn.unknown_score(query))
    d7, idx7 = knn.kneighbors(query, chunk=7)
    assert torch.equal(d7, d) and torch.equal(idx7, idx)
    # leave-one-out on the bank
    own = device_distances(knn, knn.bank_features, cuda)
    skip = np.arange(n)
    d_loo, idx_loo = knn.kneighbors(knn.bank_features, exclude_self=True, chunk=33)
    want_d, want_i = K.topk(own, n, k, skip)
    assert K.same_values(d_loo.cpu().numpy(), want_d) and np.array_equal(idx_loo.cpu().numpy(), rows[want_i])
    assert bool((idx_loo != knn.bank_rows[:, None]).all())
    loo = K.class_kth(own, n, [0, n], k, skip)[:, 0]
    knn.calibrate(tpr=0.9)
    assert knn.threshold.is_cuda and float(knn.threshold) == np.sort(loo)[int(np.ceil(0.9 * n)) - 1]
    # state dict
    again = KNN().load_state_dict(knn.state_dict())
    assert again.k == k and again.distance == distance and float(again.threshold) == float(knn.threshold)
    assert torch.equal(again.predict(query), scores)


def test_knn_bank_fraction_and_k_above_the_class_sizes(cuda):
    from openset_imagenet.knn import KNN, bank_selection
    train, gt, query = e2e_case("small")
    knn = KNN(k=1024, bank_fraction=0.3, seed=5).fit(train, gt)
    rows, start = bank_selection(gt, 0.3, 5)
    assert knn.bank_rows.cpu().numpy().tolist() == rows.tolist()
    dist = device_distances(knn, query, cuda)
    assert K.same_values(knn.predict(query).cpu().numpy(), K.class_kth(dist, len(rows), start, 1024, None, K.SIM_COSINE))
    d, idx = knn.kneighbors(query)
    assert d.shape == (50, 1024) and bool((idx[:, len(rows):] == -1).all()) and bool(torch.isinf(d[:, len(rows):]).all())
    assert np.array_equal(idx[:, :len(rows)].cpu().numpy(), rows[K.topk(dist, len(rows), 1024)[1][:, :len(rows)]])


def test_knn_arrays_writes_its_keys(cuda, tmp_path):
    from openset_imagenet.script.evaluate import knn_arrays
    from openset_imagenet import util
    train_f, gt, _ = e2e_case("small")
    logits = train_f[:, :6].copy()
    train = dict(gt=gt, logits=logits, features=train_f)
    split = dict(gt=gt[:97], logits=logits[:97], features=train_f[:97])
    knn, arrays = knn_arrays(train, split, 5, distance="cosine")
    assert sorted(arrays) == ["features", "gt", "logits", "scores", "unknown"]
    assert arrays["scores"].shape == (97, 6) and arrays["scores"].dtype == np.float32 and arrays["unknown"].shape == (97,)
    assert all(isinstance(v, np.ndarray) for v in arrays.values())
    np.savez(tmp_path / "x_knn.npz", **arrays)
    assert sorted(np.load(tmp_path / "x_knn.npz").files) == sorted(arrays)
    _, again = knn_arrays(knn, split, 5)                     # a fitted object is taken as it is
    assert again["scores"].tobytes() == arrays["scores"].tobytes() and again["unknown"].tobytes() == arrays["unknown"].tobytes()
    ccr, fpr = util.calculate_oscr(arrays["gt"], arrays["scores"], unk_label=-1)      # the scores feed the OSCR curve as they are
    assert len(ccr) == len(fpr) > 0

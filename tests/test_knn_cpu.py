"""CPU side of deep nearest neighbours (openset_imagenet/knn.py, include/osi.h ABI 24): the oracle the GPU tests compare against
(tests/knn_oracle.py) agrees with a brute-force walk of the definition on tiny inputs, the symbols are exported and declared, the C ABI
entries validate their arguments before any launch, KNN refuses bad arguments with the argument's name, the host bookkeeping of fit
(stable class sort, original row numbers, seeded fraction sampling) is right, the state dict round-trips, and evaluate.py takes and
refuses the options."""
import math
import struct

import numpy as np
import pytest
import torch

import knn_oracle as K

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- oracle
def brute_order(row, skip):
    """The definition walked literally: repeatedly take the smallest remaining column by pairwise comparison."""
    def before(a, b):                                     # does column a rank before column b?
        va, vb = np.float32(row[a]) + np.float32(0), np.float32(row[b]) + np.float32(0)
        na, nb = math.isnan(va), math.isnan(vb)
        if na != nb:
            return nb
        if not na and va != vb:
            return va < vb
        return a < b
    left = [j for j in range(len(row)) if j != skip]
    out = []
    while left:
        best = left[0]
        for j in left[1:]:
            if before(j, best):
                best = j
        out.append(best)
        left.remove(best)
    return out


TINY = np.array([[3, 1, 1, NAN, -0.0, 0.0, INF, -INF, 2, 1],
                 [NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN],
                 [5, 4, 3, 2, 1, 0, -1, -2, -3, -4],
                 [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                 [INF, NAN, INF, 1, NAN, 1, -INF, -INF, 7, 7]], dtype=np.float32)


@pytest.mark.parametrize("k", (1, 2, 3, 9, 10, 12))
@pytest.mark.parametrize("skip", (None, -1, 10, 0, 4))
def test_oracle_topk_against_a_brute_force_walk(k, skip):
    sk = None if skip is None else np.full(len(TINY), skip, dtype=np.int64)
    d, i = K.topk(TINY, 10, k, sk)
    assert d.dtype == np.float32 and i.dtype == np.int64 and d.shape == i.shape == (len(TINY), k)
    for m, row in enumerate(TINY):
        want = brute_order(row, -1 if skip is None else skip)[:k]
        assert i[m, :len(want)].tolist() == want and (i[m, len(want):] == -1).all() and np.isposinf(d[m, len(want):]).all()
        for t, j in enumerate(want):
            v = np.float32(row[j]) + np.float32(0)
            assert (math.isnan(v) and math.isnan(d[m, t])) or struct.pack("f", v) == struct.pack("f", d[m, t])


def test_oracle_order_on_a_hand_example():
    """-Inf, then -0 and +0 as one value in column order (returned as +0), the three 1s in column order, 2, 3, +Inf, NaN last."""
    d, i = K.topk(TINY[:1], 10, 10)
    assert i[0].tolist() == [7, 4, 5, 1, 2, 9, 8, 0, 6, 3]
    assert np.signbit(d[0, 1]) == np.signbit(d[0, 2]) == False and np.isnan(d[0, 9]) and d[0, 0] == -INF       # noqa: E712
    # padding columns (ld > N) never take part
    d, i = K.topk(TINY[:1], 4, 10)
    assert i[0].tolist() == [1, 2, 0, 3] + [-1] * 6


@pytest.mark.parametrize("k", (1, 2, 4))
def test_oracle_class_kth_against_a_brute_force_walk(k):
    start = np.array([0, 0, 3, 4, 4, 12, 7, 10])           # empty first, length 3, 1, empty, 4 .. 12 clamps to 10, descending pair, 7 .. 10
    for skip in (None, 3, 8):
        sk = None if skip is None else np.full(len(TINY), skip, dtype=np.int64)
        got = K.class_kth(TINY, 10, start, k, sk)
        for m, row in enumerate(TINY):
            for c in range(len(start) - 1):
                c0, c1 = min(max(start[c], 0), 10), min(max(start[c + 1], 0), 10)
                cols = [j for j in brute_order(row, -1 if skip is None else skip) if c0 <= j < c1]
                if not cols:
                    assert np.isposinf(got[m, c]), (m, c)
                else:
                    v = np.float32(row[cols[min(k, len(cols)) - 1]]) + np.float32(0)
                    assert (math.isnan(v) and math.isnan(got[m, c])) or struct.pack("f", v) == struct.pack("f", got[m, c]), (m, c)
    assert np.isposinf(K.class_kth(TINY, 10, np.array([3, 4]), 1, np.full(len(TINY), 3))).all()      # the one column is skipped


def test_oracle_transforms_by_hand():
    v = np.array([0.0, 0.5, 2.0, 3.0, -1.0, INF, NAN, -INF, 1e-45], dtype=np.float32)
    cos = K.transform(v, K.SIM_COSINE)
    assert cos[:6].tolist() == [1.0, 0.75, 0.0, 0.0, 1.0, 0.0] and np.isnan(cos[6]) and cos[7] == 1.0 and cos[8] == 1.0
    inv = K.transform(v, K.SIM_INVERSE)
    assert inv[:4].tolist() == [1.0, np.float32(1) / np.float32(1.5), np.float32(1) / np.float32(3), 0.25]
    assert np.isposinf(inv[4]) and inv[5] == 0.0 and not np.signbit(inv[5]) and np.isnan(inv[6]) and inv[7] == 0.0 and np.signbit(inv[7])
    assert K.transform(v, K.RAW).tobytes() == v.tobytes() and cos.dtype == inv.dtype == np.float32
    # one rounding for the subtraction: 1 - 0.5 * (2^-24 + 2^-48) rounds to 1 - 2^-24 ... in fp32 the product is exact
    x = np.float32(2.0 ** -23)
    assert K.transform(np.array([x]), K.SIM_COSINE)[0] == np.float32(1) - np.float32(2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 24
    for name in ("osi_knn_workspace", "osi_knn_topk", "osi_knn_class_kth"):
        assert hasattr(lib, name) and name in N.declared_symbols()
    assert (N.KNN_RAW, N.KNN_SIM_COSINE, N.KNN_SIM_INVERSE, N.KNN_MAX_K) == (K.RAW, K.SIM_COSINE, K.SIM_INVERSE, K.MAX_K) == (0, 1, 2, 1024)
    ops = N.ops()
    for name in ("knn_topk", "knn_class_kth"):
        assert hasattr(ops, name)


def test_abi_entries_validate_before_launch():
    """Each null required pointer (skip may be NULL), a size <= 0, ld below N, K of 0 / -1 / 1025, a workspace one byte short or absent,
    a bad transform: OSI_ERR_ARG, nothing launched (safe on a CPU-only host; the pointers are never dereferenced on the host)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    for args in ((0, 4, 5), (100, 0, 5), (100, 4, 0), (-1, 4, 5), (100, -2, 5), (100, 4, -7)):
        assert lib.osi_knn_workspace(*args) == 0, args
    nb = lib.osi_knn_workspace(100, 40, 5)
    assert nb > 0 and nb % 8 == 0 and lib.osi_knn_workspace(4096, 100000, 1024) % 8 == 0
    p = 4096                                             # any non-null, aligned address: argument checks come first

    def refuses(fn, good, pointers, values):
        for hole in pointers:
            args = list(good); args[hole] = None
            assert fn(*args) == -1, (fn.__name__, hole)
        for pos, value in values:
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (fn.__name__, pos, value)

    sizes = ((1, 0), (1, -1), (2, 0), (2, -1), (3, 39), (3, 0), (3, -5))
    refuses(lib.osi_knn_topk, [p, 100, 40, 40, 5, p, p, p, p, nb, None], (0, 6, 7, 8),
            sizes + ((4, 0), (4, -1), (4, 1025), (9, nb - 1), (9, 0)))
    refuses(lib.osi_knn_class_kth, [p, 100, 40, 48, p, 3, 5, p, N.KNN_SIM_COSINE, p, p, nb, None], (0, 4, 9, 10),
            sizes + ((5, 0), (5, -1), (6, 0), (6, -1), (6, 1025), (8, 3), (8, -1), (11, nb - 1), (11, 0)))


# ---------------------------------------------------------------------------------------------------------------- Python
def small_arrays(n=24, c=3, f=4, seed=0):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, c, n)
    gt[:c] = np.arange(c)
    gt[-2:] = -1
    return rng.standard_normal((n, f)).astype(np.float32), gt


def hand_state(f=4):
    return dict(bank_features=torch.arange(5 * f, dtype=torch.float32).reshape(5, f), bank_start=torch.tensor([0, 2, 2, 5]),
                bank_rows=torch.tensor([4, 7, 0, 1, 9]), bank_labels=torch.tensor([0, 0, 2, 2, 2]), k=3, distance="euclidean",
                bank_fraction=0.5, seed=7, threshold=torch.tensor(1.25))


def test_names_import_and_refuse_without_gpu():
    import openset_imagenet
    from openset_imagenet.knn import KNN
    from openset_imagenet.script.evaluate import knn_arrays
    assert openset_imagenet.KNN is KNN and "KNN" in openset_imagenet.__all__
    f, gt = small_arrays()
    knn = KNN(k=2)
    loaded = KNN().load_state_dict(hand_state())
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert knn.fit(f, gt).predict(f).shape == (24, 3) and loaded.predict(f).shape == (24, 3)
    else:
        train = dict(gt=gt, logits=f[:, :3], features=f)
        for call in (lambda: knn.fit(f, gt), lambda: loaded.predict(f), lambda: loaded.unknown_score(f), lambda: loaded.kneighbors(f),
                     lambda: loaded.calibrate(), lambda: knn_arrays(train, train, 2)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()


def test_host_side_checks_name_the_argument():
    from openset_imagenet.knn import KNN
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError, match="k must"):
            KNN(k=bad)
    for bad in (10.0, True, "3"):
        with pytest.raises(TypeError, match="k must"):
            KNN(k=bad)
    with pytest.raises(ValueError, match="distance"):
        KNN(distance="manhattan")
    for bad in (0, 0.0, -0.5, 1.5, NAN):
        with pytest.raises(ValueError, match="bank_fraction"):
            KNN(bank_fraction=bad)
    with pytest.raises(TypeError, match="bank_fraction"):
        KNN(bank_fraction="half")
    with pytest.raises(TypeError, match="seed"):
        KNN(seed=1.5)
    e = KNN()
    assert (e.k, e.distance, e.bank_fraction, e.seed, e.is_fitted, e.threshold) == (10, "cosine", 1.0, 0, False, None)
    assert (KNN(1).k, KNN(1024).k, KNN(bank_fraction=1).bank_fraction) == (1, 1024, 1.0)
    f, gt = small_arrays()
    for call in (lambda: e.predict(f), lambda: e.unknown_score(f), lambda: e.kneighbors(f), lambda: e.calibrate(), lambda: e.state_dict()):
        with pytest.raises(ValueError, match="before fit"):
            call()
    with pytest.raises(ValueError, match="number of samples"):
        e.fit(f[:-1], gt)
    with pytest.raises(ValueError, match="features"):
        e.fit(f[0], gt)
    with pytest.raises(ValueError, match="empty"):
        e.fit(f[:0], gt[:0])
    with pytest.raises(ValueError, match="no known class"):
        e.fit(f, np.full(len(gt), -1))
    with pytest.raises(ValueError, match="bank_fraction"):      # N * F * 4 >= 2^31; a view: no memory behind it
        e.fit(torch.zeros(1, 1).expand(1 << 15, 1 << 14), np.zeros(1 << 15, dtype=np.int64))
    loaded = KNN().load_state_dict(hand_state())
    for call in (loaded.predict, loaded.unknown_score, loaded.kneighbors):
        with pytest.raises(ValueError, match="features"):
            call(f[:, :3])
        with pytest.raises(ValueError, match="chunk"):
            call(f, chunk=0)
    with pytest.raises(ValueError, match="exclude_self"):
        loaded.kneighbors(f, exclude_self=True)             # 24 queries are not the bank of 5
    for bad in (0, 1.5, -1, NAN):
        with pytest.raises(ValueError, match="tpr"):
            loaded.calibrate(tpr=bad)
    with pytest.raises(TypeError, match="tpr"):
        loaded.calibrate(tpr="most")


def test_bank_selection_is_a_stable_class_sort_with_the_original_rows():
    from openset_imagenet.knn import bank_selection
    gt = np.array([2, 0, -1, 2, 0, 4, -2, 0, 2, 4])
    rows, start = bank_selection(gt)
    assert rows.tolist() == [1, 4, 7, 0, 3, 8, 5, 9] and start.tolist() == [0, 3, 3, 6, 6, 8]       # classes 1 and 3 are empty
    assert rows.dtype == start.dtype == np.int64
    # a fraction keeps ceil(f * n_c) rows per class, in row order, reproducibly from the seed
    rng = np.random.default_rng(3)
    gt = rng.integers(-1, 6, 500)
    full, full_start = bank_selection(gt)
    for frac in (0.5, 0.1, 0.999, 1e-6):
        rows, start = bank_selection(gt, frac, seed=11)
        again, again_start = bank_selection(gt, frac, seed=11)
        assert rows.tolist() == again.tolist() and start.tolist() == again_start.tolist()
        for c in range(6):
            mine, all_c = rows[start[c]:start[c + 1]], full[full_start[c]:full_start[c + 1]]
            assert len(mine) == math.ceil(frac * len(all_c)) and (np.diff(mine) > 0).all() and set(mine) <= set(all_c)
            assert (gt[mine] == c).all()
    a, b = bank_selection(gt, 0.5, seed=11)[0], bank_selection(gt, 0.5, seed=12)[0]
    assert a.tolist() != b.tolist()


def test_state_dict_round_trip(tmp_path):
    from openset_imagenet.knn import KNN
    sd = hand_state()
    knn = KNN().load_state_dict(sd)
    assert (knn.k, knn.distance, knn.bank_fraction, knn.seed, knn.is_fitted, float(knn.threshold)) == (3, "euclidean", 0.5, 7, True, 1.25)
    out = knn.state_dict()
    assert set(out) == set(sd)
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            assert out[k].device.type == "cpu" and out[k].dtype == v.dtype and torch.equal(out[k], v), k
        else:
            assert out[k] == v, k
    torch.save(out, tmp_path / "knn.pth")
    again = KNN().load_state_dict(torch.load(tmp_path / "knn.pth", weights_only=True)).state_dict()
    assert all(torch.equal(again[k], v) if isinstance(v, torch.Tensor) else again[k] == v for k, v in sd.items())
    out["bank_features"][0, 0] = 99.0                    # the loaded object owns its tensors
    assert float(knn.bank_features[0, 0]) == 0.0
    assert KNN().load_state_dict(dict(sd, threshold=None)).threshold is None
    short = dict(sd); del short["bank_rows"]
    with pytest.raises(ValueError, match="bank_rows"):
        KNN().load_state_dict(short)
    with pytest.raises(ValueError, match="bank_labels"):
        KNN().load_state_dict(dict(sd, bank_labels=torch.zeros(4, dtype=torch.int64)))
    with pytest.raises(ValueError, match="bank_start"):
        KNN().load_state_dict(dict(sd, bank_start=torch.tensor([0, 3, 2, 5])))
    with pytest.raises(ValueError, match="bank_start"):
        KNN().load_state_dict(dict(sd, bank_start=torch.tensor([0, 2, 2, 4])))
    with pytest.raises(ValueError, match="bank_features"):
        KNN().load_state_dict(dict(sd, bank_features=torch.zeros(5)))
    with pytest.raises(ValueError, match="threshold"):
        KNN().load_state_dict(dict(sd, threshold=torch.zeros(2)))
    with pytest.raises(ValueError, match="k must"):
        KNN().load_state_dict(dict(sd, k=0))


def test_evaluate_options():
    from openset_imagenet.script.evaluate import get_args
    a = get_args(["softmax", "1"])
    assert a.knn is None and a.knn_distance == "cosine" and a.knn_fraction == 1.0                # without the flag: as before
    a = get_args(["entropic", "2", "--knn", "25", "--knn-distance", "euclidean", "--knn-fraction", "0.25"])
    assert (a.knn, a.knn_distance, a.knn_fraction) == (25, "euclidean", 0.25)
    a = get_args(["entropic", "2", "--knn", "10", "--evm", "500"])
    assert (a.knn, a.evm) == (10, 500)
    with pytest.raises(SystemExit):                      # the garbage network has a background class already
        get_args(["garbage", "1", "--knn", "10"])
    with pytest.raises(SystemExit):
        get_args(["softmax", "1", "--knn-distance", "manhattan"])

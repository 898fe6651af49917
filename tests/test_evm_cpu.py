"""CPU side of the Extreme Value Machine (openset_imagenet/evm.py, include/osi.h ABI 22): the names import without a GPU and refuse to
compute there, every host-side check raises with the argument's name, the state dict round-trips, the C ABI entries validate their
arguments before any launch (the 2^31 limits of the distance kernel included), and the oracle the GPU tests compare against
(tests/evm_oracle.py) reproduces a greedy cover walked by brute force and a FitLow worked by hand."""
import numpy as np
import pytest
import torch

import evm_oracle as E
from openmax_oracle import weibull_fit


def small_arrays(n=24, c=3, f=4, seed=0):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, c, n)
    gt[:c] = np.arange(c)
    gt[-2:] = -1
    return rng.standard_normal((n, f)).astype(np.float32), gt


def hand_state(f=4):
    return dict(ev_features=torch.arange(5 * f, dtype=torch.float32).reshape(5, f),
                ev_shape=torch.tensor([1.5, 2.0, 1.0, 3.0, 2.5], dtype=torch.float64),
                ev_scale=torch.tensor([1.25, 3.0, 1.0, 2.0, 1.5], dtype=torch.float64),
                ev_shift=torch.tensor([-0.5, -0.75, -0.25, -1.0, -0.125], dtype=torch.float64),
                ev_start=torch.tensor([0, 2, 2, 5]), flags=torch.tensor([0, 1]), tailsize=20, cover_threshold=0.5,
                distance_multiplier=0.5, distance="euclidean", use_negatives=False)


def test_names_import_and_refuse_without_gpu():
    import openset_imagenet
    from openset_imagenet.evm import EVM
    from openset_imagenet.script.evaluate import evm_arrays
    assert openset_imagenet.EVM is EVM and "EVM" in openset_imagenet.__all__
    f, gt = small_arrays()
    evm = EVM(tailsize=5)
    loaded = EVM().load_state_dict(hand_state())
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert evm.fit(f, gt).predict(f).shape == (24, 3)
        assert loaded.predict(f).shape == (24, 3)
    else:
        train = dict(gt=gt, logits=f[:, :3], features=f)
        for call in (lambda: evm.fit(f, gt), lambda: loaded.predict(f), lambda: evm_arrays(train, train, 5)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()


def test_host_side_checks_name_the_argument():
    from openset_imagenet import _native as N
    from openset_imagenet.evm import EVM
    for bad in (1, 4097, 0, -3):
        with pytest.raises(ValueError, match="tailsize"):
            EVM(tailsize=bad)
    with pytest.raises(TypeError, match="tailsize"):
        EVM(tailsize=10.0)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="cover_threshold"):
            EVM(cover_threshold=bad)
    with pytest.raises(TypeError, match="cover_threshold"):
        EVM(cover_threshold="half")
    for bad in (0, -1.0, float("inf"), float("nan"), 1e-60, 1e60):
        with pytest.raises(ValueError, match="distance_multiplier"):
            EVM(distance_multiplier=bad)
    with pytest.raises(TypeError, match="distance_multiplier"):
        EVM(distance_multiplier="0.5")
    with pytest.raises(ValueError, match="distance"):
        EVM(distance="manhattan")
    e = EVM()
    assert (e.tailsize, e.cover_threshold, e.distance_multiplier, e.distance, e.use_negatives) == (1000, None, 0.5, "cosine", True)
    assert (EVM(2).tailsize, EVM(4096).tailsize, EVM(cover_threshold=1).cover_threshold) == (2, 4096, 1.0)
    f, gt = small_arrays()
    for call in (lambda: e.predict(f), lambda: e.state_dict()):
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
    # the limits fit checks before it touches the device: a class too large for the cover names the class, N * F * 4 >= 2^31
    big = np.zeros(N.EVM_MAX_COVER_ROWS + 3, dtype=np.int64)
    big[:2] = 1
    with pytest.raises(ValueError, match="class 0 has 16385 rows"):
        EVM(cover_threshold=0.5).fit(np.zeros((len(big), 2), dtype=np.float32), big)
    with pytest.raises(ValueError, match="2 GiB"):
        e.fit(torch.zeros(1, 1).expand(1 << 15, 1 << 14), np.zeros(1 << 15, dtype=np.int64))      # a view: no memory behind it
    loaded = EVM().load_state_dict(hand_state())
    with pytest.raises(ValueError, match="features"):
        loaded.predict(f[:, :3])
    with pytest.raises(ValueError, match="chunk"):
        loaded.predict(f, chunk=0)


def test_state_dict_round_trip(tmp_path):
    from openset_imagenet.evm import EVM
    sd = hand_state()
    evm = EVM().load_state_dict(sd)
    assert (evm.tailsize, evm.cover_threshold, evm.distance_multiplier, evm.distance, evm.use_negatives, evm.is_fitted) == \
        (20, 0.5, 0.5, "euclidean", False, True)
    out = evm.state_dict()
    assert set(out) == set(sd)
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            assert out[k].device.type == "cpu" and out[k].dtype == v.dtype and torch.equal(out[k], v), k
        else:
            assert out[k] == v, k
    torch.save(out, tmp_path / "evm.pth")
    again = EVM().load_state_dict(torch.load(tmp_path / "evm.pth", weights_only=True)).state_dict()
    assert all(torch.equal(again[k], v) if isinstance(v, torch.Tensor) else again[k] == v for k, v in sd.items())
    out["ev_features"][0, 0] = 99.0                      # the loaded object owns its tensors
    assert float(evm.ev_features[0, 0]) == 0.0
    assert EVM().load_state_dict(dict(sd, cover_threshold=None)).cover_threshold is None
    short = dict(sd); del short["ev_scale"]
    with pytest.raises(ValueError, match="ev_scale"):
        EVM().load_state_dict(short)
    with pytest.raises(ValueError, match="ev_shift"):
        EVM().load_state_dict(dict(sd, ev_shift=torch.zeros(4, dtype=torch.float64)))
    with pytest.raises(ValueError, match="ev_start"):
        EVM().load_state_dict(dict(sd, ev_start=torch.tensor([0, 3, 2, 5])))
    with pytest.raises(ValueError, match="ev_start"):
        EVM().load_state_dict(dict(sd, ev_start=torch.tensor([0, 2, 2, 4])))
    with pytest.raises(ValueError, match="tailsize"):
        EVM().load_state_dict(dict(sd, tailsize=1))


def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 22
    for name in ("osi_evm_workspace", "osi_evm_distances", "osi_evm_fit_rows", "osi_evm_set_cover", "osi_evm_probs"):
        assert hasattr(lib, name) and name in N.declared_symbols()
    assert (N.EVM_EUCLIDEAN, N.EVM_COSINE, N.EVM_MAX_TAIL, N.EVM_MAX_COVER_ROWS) == (0, 1, 4096, 16384)
    ops = N.ops()
    for name in ("evm_distances", "evm_fit_rows", "evm_set_cover", "evm_probs"):
        assert hasattr(ops, name)


def test_abi_entries_validate_before_launch():
    """Each null pointer, a size <= 0, ld below the row length, T of 1 and 4097, a bad metric, a multiplier of 0 / below 0 / Inf / NaN,
    a NaN threshold, R above the cover's cap, a workspace one byte short, and the three 2^31 limits of the distance kernel:
    OSI_ERR_ARG, nothing launched (safe on a CPU-only host; the pointers are never dereferenced on the host)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    for args in ((0, 4, 5), (100, 0, 5), (100, 4, 0), (-1, 4, 5), (100, -2, 5), (100, 4, -7)):
        assert lib.osi_evm_workspace(*args) == 0, args
    assert lib.osi_evm_workspace(10, 1000, 5) >= (10 + 1000) * 8
    assert lib.osi_evm_workspace(300, 10, 5) >= 300 * 5 * 8 + 300 * 4                # the cover's bit matrix and counts
    assert lib.osi_evm_workspace(16384, 10, 5) >= 16384 * 16384 // 8
    p = 4096                                             # any non-null address: argument checks come first
    inf, nan = float("inf"), float("nan")

    def refuses(fn, good, pointers, values):
        for hole in pointers:
            args = list(good); args[hole] = None
            assert fn(*args) == -1, (fn.__name__, hole)
        for pos, value in values:
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (fn.__name__, pos, value)

    need = (100 + 40) * 8
    refuses(lib.osi_evm_distances, [p, 100, p, 40, 5, N.EVM_COSINE, p, p, need, None], (0, 2, 6, 7),
            ((1, 0), (1, -1), (3, 0), (3, -1), (4, 0), (4, -1), (5, 2), (5, -1), (8, need - 1), (8, 0)))
    huge = 1 << 40
    for r, n, f in ((23171, 23171, 4), (1 << 20, 8, 512), (8, 1 << 20, 512), (1 << 16, 1 << 13, 1)):      # R N 4, R F 4, N F 4 >= 2^31
        assert max(r * n, r * f, n * f) * 4 >= 2 ** 31
        assert lib.osi_evm_distances(p, r, p, n, f, N.EVM_EUCLIDEAN, p, p, huge, None) == -1, (r, n, f)
    refuses(lib.osi_evm_fit_rows, [p, 10, 100, 100, p, 1, 20, 0.5, p, p, p, p, p, p, p, 64, None], (0, 4, 8, 9, 10, 11, 12, 13, 14),
            ((1, 0), (1, -1), (2, 0), (2, -1), (3, 99), (3, 0), (6, 1), (6, 4097), (6, 0), (6, -1), (7, 0.0), (7, -0.5), (7, inf),
             (7, nan)))
    nb = lib.osi_evm_workspace(300, 1, 1)
    refuses(lib.osi_evm_set_cover, [p, 300, p, p, p, p, 0.5, 0.5, p, p, p, nb, None], (0, 2, 3, 4, 5, 8, 9, 10),
            ((1, 0), (1, -1), (1, 16385), (6, 0.0), (6, -1.0), (6, inf), (6, nan), (7, nan), (11, 300 * 5 * 8 + 300 * 4 - 1), (11, 0)))
    refuses(lib.osi_evm_probs, [p, 100, 7, 7, p, p, p, p, 3, 0.5, p, None], (0, 4, 5, 6, 7, 10),
            ((1, 0), (1, -1), (2, 0), (2, -1), (3, 6), (8, 0), (8, -1), (9, 0.0), (9, -2.0), (9, inf), (9, nan)))


# ---------------------------------------------------------------------------------------------------------------- oracle
def brute_force_cover(cov, fitted):
    """The definition walked literally: recount every candidate's uncovered rows at every step."""
    R = len(fitted)
    U = {j for j in range(R) if fitted[j]}
    picked, order = set(), []
    while U:
        best, best_n = None, -1
        for i in range(R):
            if fitted[i] and i not in picked:
                n = sum(1 for j in U if cov[i][j])
                if n > best_n:                            # strict: the lowest index wins a tie
                    best, best_n = i, n
        picked.add(best)
        order.append(best)
        U -= {j for j in U if cov[best][j]}
    return order


HAND_COVERS = [
    # one row covers all
    ([[1, 1, 1, 1], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 0, 1]], [1, 1, 1, 1], [0]),
    # nobody covers anybody: R picks in index order
    (np.eye(5, dtype=int).tolist(), [1, 1, 1, 1, 1], [0, 1, 2, 3, 4]),
    # a tie at the first pick (rows 1 and 3 cover three each): the lower index wins, then 3 still brings 4 and 5
    ([[1, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1]],
     [1, 1, 1, 1, 1, 1], [1, 3]),
    # the second pick depends on what the first one left: row 0 covers {0,1,2,3}; of what remains row 4 covers {4,5}, row 2 only 5
    ([[1, 1, 1, 1, 0, 0], [0, 1, 0, 0, 0, 0], [0, 1, 1, 1, 0, 1], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 1]],
     [1, 1, 1, 1, 1, 1], [0, 4]),
    # unfitted rows (1 and 4) are never picked and never need covering, whatever their entries say
    ([[1, 1, 0, 0, 1], [1, 1, 1, 1, 1], [0, 0, 1, 1, 0], [0, 0, 0, 1, 0], [1, 1, 1, 1, 1]], [1, 0, 1, 1, 0], [2, 0]),
    # R = 1, and nothing fitted at all
    ([[1]], [1], [0]),
    ([[1, 1], [1, 1]], [0, 0], []),
]


@pytest.mark.parametrize("k", range(len(HAND_COVERS)))
def test_oracle_greedy_cover_against_a_brute_force_walk(k):
    cov, fitted, want = HAND_COVERS[k]
    fitted = np.asarray(fitted, dtype=bool)
    cov = np.asarray(cov, dtype=bool) & fitted[:, None] & fitted[None, :]
    assert brute_force_cover(cov, fitted) == want
    order, n = E.greedy_cover(cov, fitted)
    assert order[:n].tolist() == want and (order[n:] == -1).all() and len(order) == len(fitted)


def test_oracle_cover_matrix_uses_the_row_s_own_weibull():
    """Psi_i(d) >= threshold is asymmetric: row 0 has a wide distribution, row 1 a narrow one, row 2 is unfitted."""
    dpp = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=np.float32)
    shape, scale, shift = np.array([2.0, 2.0, 0.0]), np.array([4.0, 0.5, 0.0]), np.array([-3.0, -1.0, 0.0])
    fitted = np.array([1, 1, 0])
    p = E.psi(dpp, 0.5, shape[:, None], scale[:, None], shift[:, None], fitted[:, None].astype(bool))
    # row 0: z = -0.5 + 3 + 1 = 3.5 -> 1 - exp(-(3.5/4)^2); row 1: z = -0.5 + 1 + 1 = 1.5 -> 1 - exp(-9)
    assert abs(p[0, 1] - (1 - np.exp(-(3.5 / 4) ** 2))) < 1e-7 and abs(p[1, 0] - (1 - np.exp(-9.0))) < 1e-7 and p[2, 0] == 0
    cov = E.cover_matrix(dpp, shape, scale, shift, fitted, 0.5, 0.9)
    assert cov.tolist() == [[True, False, False], [True, True, False], [False, False, False]]
    assert E.set_cover(dpp, shape, scale, shift, fitted, 0.5, 0.9)[0].tolist() == [1, -1, -1]


def test_oracle_fit_low_on_a_hand_example():
    """One row, multiplier 0.5, T = 3. Distances to the negatives: 2, 8, 4, 6, Inf, NaN; the positive (label 1) at distance 1 takes no
    part. y = -1, -4, -2, -3; the three largest are -1, -2, -3 (the NEAREST negatives), shift = -3, x = (1, 2, 3)."""
    dist = np.array([[2, 1, 8, 4, 6, np.inf, np.nan, 77]], dtype=np.float32)          # ld = 8, N = 7: the last column is padding
    gt = np.array([0, 1, -1, 2, 5, 0, -2])
    m = E.fit_rows(dist, 7, gt, 1, 3, 0.5)
    k, lam = weibull_fit(np.array([1.0, 2.0, 3.0]))
    assert m["fitted"].tolist() == [1] and m["tail_count"].tolist() == [3] and m["shift"].tolist() == [-3.0]
    assert m["flags2"].tolist() == [2, 0] and m["shape"][0] == k and m["scale"][0] == lam
    lnx = np.log([1.0, 2.0, 3.0])                                                     # the likelihood equation, written out
    g = lambda kk: np.sum(np.exp(kk * lnx) * lnx) / np.sum(np.exp(kk * lnx)) - 1 / kk - lnx.mean()
    assert abs(g(k)) < 1e-12 and abs(lam - np.mean(np.array([1.0, 2.0, 3.0]) ** k) ** (1 / k)) < 1e-12
    # Psi at the row's own distances: nearer means more probable, beyond the tail's end it is 0
    p = E.psi(np.array([0, 2, 6, 8.5, np.nan], dtype=np.float32), 0.5, k, lam, -3.0, True)
    assert p[0] > p[1] > p[2] > 0 and p[3] == 0 and np.isnan(p[4])
    assert abs(p[1] - (1 - np.exp(-(3.0 / lam) ** k))) < 1e-7
    # T above the candidates: all four; a row with one candidate, or with equal ones, is unfitted
    assert E.fit_rows(dist, 7, gt, 1, 20, 0.5)["tail_count"].tolist() == [4]
    one = E.fit_rows(dist[:, :2], 2, gt[:2], 1, 3, 0.5)
    assert one["fitted"].tolist() == [0] and one["tail_count"].tolist() == [1] and one["flags2"].tolist() == [0, 1]
    flat = E.fit_rows(np.array([[3, 3, 3, -0.0, 0.0]], dtype=np.float32), 5, np.array([0, 0, 0, 1, 1]), 1, 3, 0.5)
    assert flat["fitted"].tolist() == [0] and flat["tail_count"].tolist() == [3]


def test_oracle_distances_and_probs_on_a_hand_example():
    a = np.array([[3, 4], [0, 0]], dtype=np.float32)
    b = np.array([[4, 3], [-3, -4], [6, 8]], dtype=np.float32)
    cos = E.distances(a, b, E.COSINE)
    assert cos[0].tolist() == [np.float32(1 - 24 / 25), 2.0, 0.0] and np.isnan(cos[1]).all()
    assert E.distances(a, b, E.EUCLIDEAN).tolist() == [[np.float32(np.sqrt(2)), 10.0, 5.0], [5.0, 5.0, 10.0]]
    # three extreme vectors, classes 0 (two), 1 (none), 2 (one)
    d = np.array([[0.5, 1.0, 2.0, 99], [np.nan, 1.0, 2.0, 99]], dtype=np.float32)
    shape, scale, shift = np.array([2.0, 2.0, 1.0]), np.array([1.0, 2.0, 1.0]), np.array([-2.0, -2.0, -2.0])
    p = E.probs(d, 3, shape, scale, shift, np.array([0, 2, 2, 3]), 0.5)
    assert p.shape == (2, 3) and p[0, 1] == 0 and p[1, 1] == 0
    assert abs(p[0, 0] - (1 - np.exp(-(2.75 ** 2)))) < 1e-7 and abs(p[0, 2] - (1 - np.exp(-2.0))) < 1e-7
    assert np.isnan(p[1, 0]) and p[1, 2] == p[0, 2]


def test_evaluate_options():
    from openset_imagenet.script.evaluate import get_args
    a = get_args(["softmax", "1"])
    assert a.evm is None and a.evm_cover is None and a.evm_multiplier == 0.5 and a.evm_distance == "cosine"    # without the flag: as before
    a = get_args(["entropic", "2", "--evm", "500", "--evm-cover", "0.7", "--evm-multiplier", "0.25", "--evm-distance", "euclidean"])
    assert (a.evm, a.evm_cover, a.evm_multiplier, a.evm_distance) == (500, 0.7, 0.25, "euclidean")
    a = get_args(["entropic", "2", "--evm", "500", "--openmax", "100"])
    assert (a.evm, a.openmax) == (500, 100)
    with pytest.raises(SystemExit):                      # the garbage network has a background class already
        get_args(["garbage", "1", "--evm", "500"])
    with pytest.raises(SystemExit):
        get_args(["softmax", "1", "--evm-distance", "manhattan"])

"""CPU side of OpenMax (openset_imagenet/openmax.py, include/osi.h ABI 21): the names import without a GPU and refuse to compute
there, every host-side check raises with the argument's name, the state dict round-trips, the C ABI entries validate their
arguments before any launch, and the oracle the GPU tests compare against (tests/openmax_oracle.py) agrees with scipy's Weibull
fit, does not depend on the order of its data, and reproduces a recalibration worked by hand."""
import numpy as np
import pytest
import torch

import openmax_oracle as O


def small_arrays(n=12, c=3, f=4, seed=0):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, c, n)
    logits = rng.standard_normal((n, c)).astype(np.float32)
    logits[np.arange(n), gt] += 4
    return rng.standard_normal((n, f)).astype(np.float32), logits, gt


def hand_state(c=3, f=4):
    return dict(mav=torch.arange(c * f, dtype=torch.float32).reshape(c, f), shape=torch.tensor([1.5, 2.0, 0.0], dtype=torch.float64),
                scale=torch.tensor([1.25, 3.0, 0.0], dtype=torch.float64), shift=torch.tensor([0.5, 0.75, 0.0], dtype=torch.float64),
                fitted=torch.tensor([1, 1, 0], dtype=torch.uint8), count=torch.tensor([5, 4, 1]), tail_count=torch.tensor([5, 4, 1]),
                flags=torch.tensor([0, 1]), tailsize=20, distance="cosine", alpha=2)


def test_names_import_and_refuse_without_gpu():
    import openset_imagenet
    from openset_imagenet.openmax import OpenMax
    from openset_imagenet.script.evaluate import openmax_arrays
    assert openset_imagenet.OpenMax is OpenMax
    f, lg, gt = small_arrays()
    om = OpenMax(tailsize=5)
    loaded = OpenMax().load_state_dict(hand_state())
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert om.fit(f, lg, gt).predict(lg, f).shape == (12, 4)
        assert loaded.w_scores(f).shape == (12, 3)
    else:
        train = dict(gt=gt, logits=lg, features=f)
        for call in (lambda: om.fit(f, lg, gt), lambda: loaded.predict(lg, f), lambda: loaded.w_scores(f),
                     lambda: openmax_arrays(train, train, 5, 3, "euclidean")):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()


def test_host_side_checks_name_the_argument():
    from openset_imagenet.openmax import OpenMax
    for bad in (1, 4097, 0, -3):
        with pytest.raises(ValueError, match="tailsize"):
            OpenMax(tailsize=bad)
    with pytest.raises(TypeError, match="tailsize"):
        OpenMax(tailsize=10.0)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="alpha"):
            OpenMax(alpha=bad)
    with pytest.raises(TypeError, match="alpha"):
        OpenMax(alpha=2.5)
    with pytest.raises(ValueError, match="distance"):
        OpenMax(distance="manhattan")
    assert (OpenMax(2).tailsize, OpenMax(4096).tailsize, OpenMax(alpha=1).alpha) == (2, 4096, 1)
    f, lg, gt = small_arrays()
    om = OpenMax()
    for call in (lambda: om.predict(lg, f), lambda: om.w_scores(f), lambda: om.state_dict()):
        with pytest.raises(ValueError, match="before fit"):
            call()
    with pytest.raises(ValueError, match="number of samples"):
        om.fit(f[:-1], lg, gt)
    with pytest.raises(ValueError, match="number of samples"):
        om.fit(f, lg, gt[:-1])
    with pytest.raises(ValueError, match="features"):
        om.fit(f[0], lg, gt)
    with pytest.raises(ValueError, match="empty"):
        om.fit(f[:0], lg[:0], gt[:0])
    loaded = OpenMax().load_state_dict(hand_state())
    with pytest.raises(ValueError, match="logits"):
        loaded.predict(lg[:, :2], f)
    with pytest.raises(ValueError, match="features"):
        loaded.predict(lg, f[:, :3])
    with pytest.raises(ValueError, match="features"):
        loaded.w_scores(f[:, :3])
    with pytest.raises(ValueError, match="number of samples"):
        loaded.predict(lg, f[:-1])


def test_state_dict_round_trip(tmp_path):
    from openset_imagenet.openmax import OpenMax
    sd = hand_state()
    om = OpenMax().load_state_dict(sd)
    assert (om.tailsize, om.distance, om.alpha, om.is_fitted) == (20, "cosine", 2, True)
    out = om.state_dict()
    assert set(out) == set(sd)
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            assert out[k].device.type == "cpu" and out[k].dtype == v.dtype and torch.equal(out[k], v), k
        else:
            assert out[k] == v, k
    torch.save(out, tmp_path / "om.pth")
    again = OpenMax().load_state_dict(torch.load(tmp_path / "om.pth", weights_only=True)).state_dict()
    assert all(torch.equal(again[k], v) if isinstance(v, torch.Tensor) else again[k] == v for k, v in sd.items())
    out["mav"][0, 0] = 99.0                              # the loaded object owns its tensors
    assert float(om.mav[0, 0]) == 0.0
    short = dict(sd); del short["scale"]
    with pytest.raises(ValueError, match="scale"):
        OpenMax().load_state_dict(short)
    wrong = dict(sd, shift=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="shift"):
        OpenMax().load_state_dict(wrong)
    with pytest.raises(ValueError, match="tailsize"):
        OpenMax().load_state_dict(dict(sd, tailsize=1))


def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 21
    for name in ("osi_openmax_workspace", "osi_openmax_class_means", "osi_openmax_distances", "osi_openmax_fit_tails",
                 "osi_openmax_wscores", "osi_openmax_recalibrate"):
        assert hasattr(lib, name) and name in N.declared_symbols()
    assert (N.OPENMAX_EUCLIDEAN, N.OPENMAX_COSINE, N.OPENMAX_MAX_TAIL) == (0, 1, 4096)
    ops = N.ops()
    for name in ("openmax_class_means", "openmax_distances", "openmax_fit_tails", "openmax_wscores", "openmax_recalibrate"):
        assert hasattr(ops, name)


def test_abi_entries_validate_before_launch():
    """Each null pointer, N / C / F <= 0, T of 1 and 4097, a bad metric, alpha 0, C above the ranking cap, a workspace one byte
    short: OSI_ERR_ARG, nothing launched (safe on a CPU-only host; the pointers are never dereferenced on the host)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    for args in ((0, 4, 5), (100, 0, 5), (100, 4, 0), (-1, 4, 5), (100, -2, 5), (100, 4, -7)):
        assert lib.osi_openmax_workspace(*args) == 0, args
    nb = lib.osi_openmax_workspace(100, 4, 5)
    assert nb > 0
    p = 4096                                             # any non-null address: argument checks come first

    def refuses(fn, good, pointers, values):
        for hole in pointers:
            args = list(good); args[hole] = None
            assert fn(*args) == -1, (fn.__name__, hole)
        for pos, value in values:
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (fn.__name__, pos, value)

    refuses(lib.osi_openmax_class_means, [p, p, p, 100, 4, 5, p, p, p, p, nb, None], (0, 1, 2, 6, 7, 8, 9),
            ((3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, -1), (10, nb - 1), (10, 0)))
    for cls in (None, p):
        refuses(lib.osi_openmax_distances, [p, p, cls, 100, 4, 5, N.OPENMAX_EUCLIDEAN, p, None], (0, 1, 7),
                ((3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, -1), (6, 2), (6, -1)))
    refuses(lib.osi_openmax_fit_tails, [p, p, p, 100, 4, 20, p, p, p, p, p, p, p, nb, None], (0, 1, 2, 6, 7, 8, 9, 10, 11, 12),
            ((3, 0), (3, -1), (4, 0), (4, -1), (5, 1), (5, 4097), (5, 0), (5, -1), (13, nb - 1), (13, 0)))
    refuses(lib.osi_openmax_wscores, [p, 100, 4, p, p, p, p, p, None], (0, 3, 4, 5, 6, 7), ((1, 0), (1, -1), (2, 0), (2, -1)))
    refuses(lib.osi_openmax_recalibrate, [p, p, 100, 4, 3, p, None], (0, 1, 5),
            ((2, 0), (2, -1), (3, 0), (3, -1), (4, 0), (4, -1), (3, 2049)))


# ---------------------------------------------------------------------------------------------------------------- oracle
def tail_sample(n, spread, seed):
    """n values x >= 1 as the fit sees them: x - min + 1 of fp32 distances from 10 to 10 * (1 + spread), Weibull-distributed between."""
    rng = np.random.default_rng(seed)
    u = rng.weibull(1.7, n)
    u = (u - u.min()) / (u.max() - u.min())
    d = np.sort((10.0 * (1 + spread * u)).astype(np.float32).astype(np.float64))
    return d - d[0] + 1.0


SCIPY_CASES = [(n, spread) for n in (2, 20, 100, 1000, 4096) for spread in (1e-3, 0.05, 1.0)]


@pytest.mark.parametrize("n,spread", SCIPY_CASES)
def test_oracle_agrees_with_scipy(n, spread):
    """weibull_min.fit(x, floc=0) is the same maximum-likelihood problem; scipy's optimiser stops at 2e-6 .. 6e-6 relative on these
    sizes, so 1e-4 separates a wrong equation from its stopping rule. Relative spreads below 1e-3 are left out: scipy is unreliable
    there."""
    stats = pytest.importorskip("scipy.stats")
    x = tail_sample(n, spread, seed=n)
    assert len(x) == n and (x.max() - x.min()) / 10.0 >= 0.999e-3
    k, lam = O.weibull_fit(x)
    k_ref, _, lam_ref = stats.weibull_min.fit(x, floc=0)
    assert abs(k - k_ref) <= 1e-4 * k_ref and abs(lam - lam_ref) <= 1e-4 * lam_ref, (k, k_ref, lam, lam_ref)


def test_oracle_root_is_order_free():
    """The oracle sums with numpy in whatever order the data come; 20 random permutations move k and lambda by less than 1e-13
    relative (measured: <= 2e-15). The device sums a sorted tail in a fixed tree: its bar of 1e-9 sits far above this noise."""
    worst = 0.0
    for n, spread in ((20, 1e-3), (100, 0.05), (1000, 1.0), (4096, 1e-3)):
        x = tail_sample(n, spread, seed=7 + n)
        k0, l0 = O.weibull_fit(x)
        rng = np.random.default_rng(n)
        for _ in range(20):
            k, lam = O.weibull_fit(rng.permutation(x))
            worst = max(worst, abs(k - k0) / k0, abs(lam - l0) / l0)
    assert worst < 1e-13, worst


def test_oracle_fit_satisfies_the_likelihood_equation():
    x = tail_sample(100, 0.05, seed=3)
    k, lam = O.weibull_fit(x)
    lnx = np.log(x)
    assert O.weibull_g(np.nextafter(k, 0), lnx) <= 0 <= O.weibull_g(np.nextafter(k, np.inf), lnx) or abs(O.weibull_g(k, lnx)) < 1e-14
    assert abs(lam - np.mean(x ** k) ** (1 / k)) <= 1e-12 * lam


def test_recalibration_worked_by_hand():
    """Two rows, C = 3, alpha = 2 (a = 2), dyadic numbers.
    Row 0: v = (2, 4, 1), w = (0.5, 0.25, 1). Ranks: column 1 (r = 0), column 0 (r = 1). omega_1 = 1 - 0.25 * 2/2 = 0.75,
      omega_0 = 1 - 0.5 * 1/2 = 0.75, omega_2 = 1. v^ = (1.5, 3, 1), v^_unk = 2 * 0.25 + 4 * 0.25 = 1.5.
    Row 1: v = (1, 1, -2), w = (1, 0.5, 0.5): the tie ranks column 0 first. omega_0 = 1 - 1 * 2/2 = 0, omega_1 = 1 - 0.5 * 1/2 = 0.75.
      v^ = (0, 0.75, -2), v^_unk = 1 * 1 + 1 * 0.25 = 1.25."""
    v = np.array([[2, 4, 1], [1, 1, -2]], dtype=np.float32)
    w = np.array([[0.5, 0.25, 1], [1, 0.5, 0.5]], dtype=np.float32)
    hat = np.array([[1.5, 3, 1, 1.5], [0, 0.75, -2, 1.25]])
    want = np.exp(hat) / np.exp(hat).sum(1, keepdims=True)
    got = O.recalibrate(v, w, 2)
    assert got.dtype == np.float32 and got.shape == (2, 4)
    assert np.abs(got - want).max() < 1e-7
    # alpha above C clamps: a = 3 for alpha = 8
    assert np.array_equal(O.recalibrate(v, w, 8), O.recalibrate(v, w, 3))
    # alpha = 1: only the top column moves
    hat1 = np.array([[2, 3, 1, 1], [0, 1, -2, 1]])
    assert np.abs(O.recalibrate(v, w, 1) - np.exp(hat1) / np.exp(hat1).sum(1, keepdims=True)).max() < 1e-7
    # a NaN logit row is NaN throughout, its neighbour is untouched
    v2 = v.copy(); v2[0, 2] = np.nan
    got2 = O.recalibrate(v2, w, 2)
    assert np.isnan(got2[0]).all() and np.array_equal(got2[1], got[1])


def test_oracle_stages_on_a_hand_example():
    """Four rows, C = 2, F = 2: rows 0 and 2 are correct for class 0, row 1 is wrong, row 3 has a negative label."""
    f = np.array([[1, 3], [5, 5], [3, -1], [7, 7]], dtype=np.float32)
    lg = np.array([[2, 1], [3, 0], [1, 1], [9, 0]], dtype=np.float32)     # row 2: a tie, the first maximum is column 0
    gt = np.array([0, 1, 0, -1])
    mav, count, correct = O.class_means(f, lg, gt)
    assert correct.tolist() == [True, False, True, False] and count.tolist() == [2, 0]
    assert mav.tolist() == [[2, 1], [0, 0]]
    d = O.distances(f, mav, None, O.EUCLIDEAN)
    assert d[0].tolist() == [np.float32(np.sqrt(5)), np.float32(np.sqrt(10))]
    assert O.distances(f, mav, gt, O.EUCLIDEAN)[[0, 2]].tolist() == [np.float32(np.sqrt(5))] * 2 and np.isnan(O.distances(f, mav, gt, 0)[3])
    cos = O.distances(f, mav, np.array([0, 0, 0, 0]), O.COSINE)
    assert cos[0] == np.float32(1 - 5 / np.sqrt(10 * 5)) and np.isnan(O.distances(f, mav, np.array([1, 1, 1, 1]), O.COSINE)).all()
    fit = O.fit_tails(np.array([1, 9, 1, 9], dtype=np.float32), gt, correct, 2, 5)
    assert fit["fitted"].tolist() == [0, 0] and fit["tail_count"].tolist() == [2, 0] and fit["flags2"].tolist() == [0, 2]


def test_recorded_end_to_end_movement_holds():
    """The bar of the real-valued end-to-end GPU test is four times the largest movement of the oracle's own probs under +-1 ulp
    of its fp32 distances; the recorded value (test_openmax_gpu.E2E_MEASURED) must cover what these inputs give."""
    from test_openmax_gpu import E2E_ALPHA, E2E_CASES, E2E_MEASURED, E2E_REAL_BAR, E2E_TAIL
    worst = 0.0
    for shape, metric in E2E_CASES:
        f, lg, gt = O.make_case(*shape, seed=shape[0] + shape[2], integer=False)
        worst = max(worst, O.jitter_movement(f, lg, gt, E2E_TAIL, metric, E2E_ALPHA))
    print(f"largest movement {worst:.3e}")
    assert 0.5 * E2E_MEASURED <= worst <= E2E_MEASURED and E2E_REAL_BAR == 4 * E2E_MEASURED


def test_evaluate_options():
    from openset_imagenet.script.evaluate import get_args
    a = get_args(["softmax", "1"])
    assert a.openmax is None and a.openmax_alpha == 3 and a.openmax_distance == "euclidean"      # without the flag: today's run
    a = get_args(["entropic", "2", "--openmax", "500", "--openmax-alpha", "5", "--openmax-distance", "cosine"])
    assert (a.openmax, a.openmax_alpha, a.openmax_distance) == (500, 5, "cosine")
    with pytest.raises(SystemExit):                      # the garbage network has a background class already
        get_args(["garbage", "1", "--openmax", "500"])
    with pytest.raises(SystemExit):
        get_args(["softmax", "1", "--openmax-distance", "manhattan"])

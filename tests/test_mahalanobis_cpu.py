"""CPU side of the Mahalanobis scores (openset_imagenet/mahalanobis.py, include/osi.h ABI 25): the oracle the GPU tests compare against
(tests/mahalanobis_oracle.py) agrees with brute-force per-row quadratic forms through np.linalg.inv on a tiny case, the symbols are
exported and declared, every C ABI entry validates its arguments before any launch, Mahalanobis refuses bad arguments by name, the
state dict round-trips, and evaluate.py takes and refuses the options."""
import math

import numpy as np
import pytest
import torch

import mahalanobis_oracle as O

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- oracle
def tiny(seed=0, n=40, c=3, f=5):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, c, n)
    gt[:c] = np.arange(c)
    gt[-3:] = (-1, -2, c)                                 # a negative, another one, a label past the classes: none is counted
    x = (rng.standard_normal((n, f)) + 2.0 * gt[:, None]).astype(np.float32)
    return x, gt, c


@pytest.mark.parametrize("relative", (False, True))
@pytest.mark.parametrize("shrinkage", (0.0, 0.25, 1.0))
def test_oracle_against_brute_force_quadratic_forms(shrinkage, relative):
    x, gt, c = tiny()
    gt2 = gt.copy()
    gt2[-1] = 1                                           # C = max(gt) + 1 = 3; the two negative rows stay
    fit = O.Fit(x, gt2, shrinkage, relative)
    keep = gt2 >= 0
    xs, ys = x[keep].astype(np.float64), gt2[keep]
    mu = np.stack([xs[ys == k].mean(axis=0) for k in range(c)])
    a = xs - mu[ys]
    n, f = len(xs), x.shape[1]
    cov = a.T @ a / n
    cov = (1 - shrinkage) * cov + shrinkage * np.trace(cov) / f * np.eye(f)
    inv = np.linalg.inv(cov)
    q = x[:7].astype(np.float64)
    want = np.array([[(r - mu[k]) @ inv @ (r - mu[k]) for k in range(c)] for r in q])
    if relative:
        mu0 = xs.mean(axis=0)
        a0 = xs - mu0
        cov0 = a0.T @ a0 / n
        cov0 = (1 - shrinkage) * cov0 + shrinkage * np.trace(cov0) / f * np.eye(f)
        inv0 = np.linalg.inv(cov0)
        want = want - np.array([(r - mu0) @ inv0 @ (r - mu0) for r in q])[:, None]
    got = fit.distances(q)
    assert fit.info == 0 and got.shape == (7, c)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9)
    assert np.allclose(fit.logdet, np.linalg.slogdet(cov)[1], rtol=1e-12, atol=1e-12)
    assert np.allclose(fit.L @ fit.L.T, cov, rtol=1e-12, atol=1e-12) and np.allclose(fit.W @ fit.L, np.eye(f), atol=1e-12)
    assert (np.triu(fit.L, 1) == 0).all() and (np.triu(fit.W, 1) == 0).all()
    p = fit.predict(q)
    if relative:
        assert np.allclose(p, 1 / (1 + np.exp(want / (2 * f)))) and ((p > 0) & (p < 1)).all()
    else:
        assert np.allclose(p, np.exp(-want / (2 * f))) and ((p > 0) & (p <= 1)).all()
    assert np.array_equal(fit.unknown_score(q), got.min(axis=1))


def test_oracle_ignores_uncounted_rows_and_empty_classes():
    x, gt, c = tiny(1)
    gt[gt == 1] = 0                                       # class 1 is empty
    mean, count = O.class_means(x, gt, c)
    assert count.tolist() == [int((gt == 0).sum()), 0, int((gt == 2).sum()), int(((gt >= 0) & (gt < c)).sum())]
    assert (mean[1] == 0).all() and np.allclose(mean[c], x[(gt >= 0) & (gt < c)].astype(np.float64).mean(axis=0))
    keep = (gt >= 0) & (gt < c)
    for mode in (O.WITHIN, O.TOTAL):
        assert np.array_equal(O.scatter(x, gt, mean, c, mode), O.scatter(x[keep], gt[keep], mean, c, mode))
    s = O.scatter(x, gt, mean, c, O.TOTAL)
    assert np.array_equal(s, s.T)


def test_oracle_factor_failure_and_transforms():
    L, W, logdet, info = O.factor(np.zeros((4, 4)), 1.0, 0.0)
    assert info == 1 and not L.any() and not W.any() and math.isnan(logdet)
    s = np.diag([1.0, 2.0, 0.0, 3.0])
    assert O.factor(s, 1.0, 0.0)[3] == 3 and O.factor(s, 1.0, 0.5)[3] == 0
    s[0, 0] = NAN
    assert O.factor(s, 1.0, 0.5)[3] == 1
    v = np.array([0.0, 8.0, -8.0, INF, NAN])
    g = O.transform(v, O.SIM_GAUSS, 4)
    assert g[:4].tolist() == [1.0, math.exp(-1.0), 1.0, 0.0] and math.isnan(g[4])
    lg = O.transform(v, O.SIM_LOGISTIC, 4)
    assert lg[:4].tolist() == [0.5, 1 / (1 + math.e), 1 / (1 + math.exp(-1.0)), 0.0] and math.isnan(lg[4])
    assert np.array_equal(O.sqdist(np.array([[1.0, 2.0]]), np.array([[0.0, 0.0], [1.0, 2.0]]), np.array([0.5])), [[4.5, -0.5]])


# ------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("osi_maha_workspace", "osi_maha_class_means", "osi_maha_scatter", "osi_maha_factor", "osi_maha_whiten_f32",
         "osi_maha_whiten_f64", "osi_maha_sqdist")


def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 25
    for name in NAMES:
        assert hasattr(lib, name) and name in N.declared_symbols()
    assert (N.MAHA_WITHIN, N.MAHA_TOTAL) == (O.WITHIN, O.TOTAL) == (0, 1)
    assert (N.MAHA_RAW, N.MAHA_SIM_GAUSS, N.MAHA_SIM_LOGISTIC) == (O.RAW, O.SIM_GAUSS, O.SIM_LOGISTIC) == (0, 1, 2)
    assert N.MAHA_MAX_F == O.MAX_F == 32768
    ops = N.ops()
    for name in ("maha_class_means", "maha_scatter", "maha_factor", "maha_whiten", "maha_sqdist"):
        assert hasattr(ops, name)


def test_abi_entries_validate_before_launch():
    """Each null required pointer (minus may be NULL), a size <= 0, sizes past the limits, a bad enum, shrinkage outside [0, 1] or NaN,
    a scale that is not positive and finite, both or neither output of sqdist, a workspace one byte short, absent or misaligned:
    OSI_ERR_ARG, nothing launched (safe on a CPU-only host; the pointers are never dereferenced on the host)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    for args in ((0, 4, 5), (100, 0, 5), (100, 4, 0), (-1, 4, 5), (100, -2, 5), (100, 4, -7), (100, 4, N.MAHA_MAX_F + 1)):
        assert lib.osi_maha_workspace(*args) == 0, args
    nb = lib.osi_maha_workspace(1000, 4, 40)
    assert nb > 64 and nb % 8 == 0 and lib.osi_maha_workspace(100000, 116, 2048) % 8 == 0
    assert lib.osi_maha_workspace(1000, 4, 40) == lib.osi_maha_workspace(1000, 9, 40)     # the class count sizes nothing
    p = 4096                                             # any non-null, aligned address: argument checks come first

    def refuses(fn, good, pointers, values):
        for hole in pointers:
            args = list(good); args[hole] = None
            assert fn(*args) == -1, (fn.__name__, hole)
        for pos, value in values:
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (fn.__name__, pos, value)

    big = 1 << 20                                        # big * 2048 = 2^31 elements: one past the limit
    refuses(lib.osi_maha_class_means, [p, p, 1000, 4, 40, p, p, p, nb, None], (0, 1, 5, 6, 7),
            ((2, 0), (2, -1), (3, 0), (3, -1), (4, 0), (4, -1), (4, N.MAHA_MAX_F + 1), (8, 63), (8, 0), (7, p + 4)))
    assert lib.osi_maha_class_means(p, p, big, 4, 2048, p, p, p, 1 << 40, None) == -1
    assert lib.osi_maha_class_means(p, p, 10, big, 2048, p, p, p, 1 << 40, None) == -1
    refuses(lib.osi_maha_scatter, [p, p, p, 1000, 4, 40, N.MAHA_WITHIN, 0, p, p, nb, None], (0, 1, 2, 8, 9),
            ((3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, -1), (5, N.MAHA_MAX_F + 1), (6, 2), (6, -1), (7, 2), (7, -1), (10, nb - 1),
             (10, 64), (10, 0), (9, p + 4)))
    assert lib.osi_maha_scatter(p, p, p, big, 4, 2048, 0, 0, p, p, 1 << 40, None) == -1
    refuses(lib.osi_maha_factor, [p, 40, 0.5, 0.1, p, p, p, p, p, nb, None], (0, 4, 5, 6, 7, 8),
            ((1, 0), (1, -1), (1, N.MAHA_MAX_F + 1), (2, 0.0), (2, -1.0), (2, INF), (2, NAN), (3, -1e-9), (3, 1.0 + 1e-9), (3, NAN), (3, INF),
             (9, 63), (9, 0), (8, p + 4)))
    for fn in (lib.osi_maha_whiten_f32, lib.osi_maha_whiten_f64):
        refuses(fn, [p, 100, 40, p, p, p, nb, None], (0, 3, 4, 5), ((1, 0), (1, -1), (2, 0), (2, -1), (2, N.MAHA_MAX_F + 1), (1, big * 64),
                                                                     (6, 63), (6, 0), (5, p + 4)))
        assert fn(p, big, 2048, p, p, p, 1 << 40, None) == -1
    good = [p, 100, p, 4, 40, None, N.MAHA_RAW, p, None, p, nb, None]
    refuses(lib.osi_maha_sqdist, good, (0, 2, 7, 9),
            ((1, 0), (1, -1), (3, 0), (3, -1), (4, 0), (4, -1), (4, N.MAHA_MAX_F + 1), (6, 3), (6, -1), (8, p), (10, 63), (10, 0), (9, p + 4)))
    both = list(good); both[7] = None; both[8] = p          # the fp64 output alone is fine as far as the checks go: only sizes can refuse it
    bad = list(both); bad[1] = 0
    assert lib.osi_maha_sqdist(*bad) == -1
    assert lib.osi_maha_sqdist(p, big, p, 4, 2048, None, 0, p, None, p, 1 << 40, None) == -1
    assert lib.osi_maha_sqdist(p, 1 << 16, p, 1 << 15, 8, None, 0, p, None, p, 1 << 40, None) == -1      # M * C = 2^31


# ---------------------------------------------------------------------------------------------------------------- Python
def hand_state(relative, f=3, c=2):
    eye = torch.eye(f, dtype=torch.float64)
    sd = dict(means=torch.arange((c + 1) * f, dtype=torch.float64).reshape(c + 1, f), counts=torch.tensor([4, 6, 10]), L=2 * eye,
              W=0.5 * eye, logdet=torch.tensor([2 * f * math.log(2.0)], dtype=torch.float64),
              whitened_means=0.5 * torch.arange(c * f, dtype=torch.float64).reshape(c, f), L0=None, W0=None, logdet0=None,
              whitened_mean0=None, shrinkage=0.25, relative=relative)
    if relative:
        sd.update(L0=4 * eye, W0=0.25 * eye, logdet0=torch.tensor([2 * f * math.log(4.0)], dtype=torch.float64),
                  whitened_mean0=torch.ones(1, f, dtype=torch.float64))
    return sd


def test_names_import_and_refuse_without_gpu():
    import openset_imagenet
    from openset_imagenet.mahalanobis import Mahalanobis
    from openset_imagenet.script.evaluate import mahalanobis_arrays
    assert openset_imagenet.Mahalanobis is Mahalanobis and "Mahalanobis" in openset_imagenet.__all__
    x, gt, c = tiny()
    x3 = x[:, :3]
    maha = Mahalanobis(shrinkage=0.1)
    loaded = Mahalanobis().load_state_dict(hand_state(True))
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert maha.fit(x, gt).predict(x).shape == (len(x), c + 1) and loaded.distances(x3).shape == (len(x), 2)
    else:
        train = dict(gt=gt, logits=x[:, :3], features=x)
        for call in (lambda: maha.fit(x, gt), lambda: loaded.predict(x3), lambda: loaded.distances(x3), lambda: loaded.unknown_score(x3),
                     lambda: mahalanobis_arrays(train, train, 0.1)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()


def test_host_side_checks_name_the_argument():
    from openset_imagenet.mahalanobis import Mahalanobis
    for bad in (-0.1, 1.5, NAN, INF):
        with pytest.raises(ValueError, match="shrinkage must"):
            Mahalanobis(shrinkage=bad)
    for bad in ("0.1", None, True):
        with pytest.raises(TypeError, match="shrinkage must"):
            Mahalanobis(shrinkage=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="relative must"):
            Mahalanobis(relative=bad)
    m = Mahalanobis(shrinkage=1, relative=True)
    assert m.shrinkage == 1.0 and isinstance(m.shrinkage, float) and m.relative is True and not m.is_fitted
    x, gt, _ = tiny()
    for call, what in ((lambda: m.predict(x), "predict"), (lambda: m.distances(x), "distances"), (lambda: m.unknown_score(x), "unknown_score"),
                       (lambda: m.state_dict(), "state_dict")):
        with pytest.raises(ValueError, match=f"{what} before fit"):
            call()
    # shape checks come before any GPU work: they raise ValueError on a host without a GPU too
    with pytest.raises(ValueError, match="features must be a matrix"):
        m.fit(x[0], gt[:1])
    with pytest.raises(ValueError, match="disagree on the number of samples"):
        m.fit(x, gt[:-1])
    with pytest.raises(ValueError, match="must not be empty"):
        m.fit(x[:0], gt[:0])
    with pytest.raises(ValueError, match="chunk must"):
        m.fit(x, gt, chunk=0)
    loaded = Mahalanobis().load_state_dict(hand_state(False))
    with pytest.raises(ValueError, match=r"features must be \[M, 3\]"):
        loaded.predict(x)
    with pytest.raises(ValueError, match="chunk must"):
        loaded.distances(x[:, :3], chunk=-2)


@pytest.mark.parametrize("relative", (False, True))
def test_state_dict_bookkeeping(relative):
    from openset_imagenet.mahalanobis import Mahalanobis
    sd = hand_state(relative)
    m = Mahalanobis().load_state_dict(sd)
    assert m.is_fitted and m.shrinkage == 0.25 and m.relative is relative
    assert m.W.dtype == torch.float64 and m.counts.dtype == torch.int64 and m.W.device.type == "cpu"
    assert (m.W0 is None) == (not relative)
    back = m.state_dict()
    assert set(back) == set(sd)
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(back[k], v.to(back[k].dtype)), k
            assert back[k].data_ptr() != getattr(m, k).data_ptr()                     # copies, not views
        else:
            assert back[k] == v, k
    again = Mahalanobis(shrinkage=0.9).load_state_dict(back)
    assert again.shrinkage == 0.25 and torch.equal(again.L, m.L)
    for drop in ("W", "relative", "whitened_mean0"):
        with pytest.raises(ValueError, match="lacks"):
            Mahalanobis().load_state_dict({k: v for k, v in sd.items() if k != drop})
    wrong = dict(sd, L=torch.eye(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="L must have shape"):
        Mahalanobis().load_state_dict(wrong)
    with pytest.raises(ValueError, match="counts must have shape"):
        Mahalanobis().load_state_dict(dict(sd, counts=torch.tensor([1, 2])))
    if relative:
        with pytest.raises(ValueError, match="no tensor for"):
            Mahalanobis().load_state_dict(dict(sd, W0=None))
    else:                                                 # background entries of a plain model are not read
        assert Mahalanobis().load_state_dict(dict(sd, W0=torch.zeros(1))).W0 is None


def test_evaluate_takes_and_refuses_the_options():
    from openset_imagenet.script.evaluate import get_args
    a = get_args(["entropic", "2"])
    assert a.mahalanobis is False and a.mahalanobis_shrinkage == 0.0 and a.mahalanobis_relative is False
    a = get_args(["softmax", "1", "--mahalanobis", "--mahalanobis-shrinkage", "0.05", "--mahalanobis-relative", "--knn", "10"])
    assert a.mahalanobis is True and a.mahalanobis_shrinkage == 0.05 and a.mahalanobis_relative is True and a.knn == 10
    for bad in (["garbage", "1", "--mahalanobis"], ["softmax", "1", "--mahalanobis", "--mahalanobis-shrinkage", "1.5"],
                ["softmax", "1", "--mahalanobis-shrinkage", "-0.1"], ["softmax", "1", "--mahalanobis-shrinkage", "nan"]):
        with pytest.raises(SystemExit):
            get_args(bad)

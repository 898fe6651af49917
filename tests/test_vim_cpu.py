"""CPU side of ViM and its eigensolver (openset_imagenet/vim.py, include/osi.h ABI 26): the oracle the GPU tests compare against
(tests/vim_oracle.py) agrees with a brute-force ViM through an explicit projector on a tiny case, its numpy restatement of the device's
Jacobi converges on every eigensolver input of the GPU tests, the symbols are exported and declared, every C ABI entry validates its
arguments before any launch, ViM refuses bad arguments by name, the state dict round-trips, and evaluate.py takes and refuses the
options."""
import numpy as np
import pytest
import torch

import vim_oracle as O

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- oracle
def tiny(seed=0, n=50, c=3, f=6):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, f)) * np.array([3.0, 2.5, 2.0, 0.4, 0.3, 0.2]) + 1.0).astype(np.float32)
    logits = rng.standard_normal((n, c)).astype(np.float32) * 2
    gt = rng.integers(0, c, n)
    gt[-3:] = (-1, -2, -1)
    return x, logits, gt


@pytest.mark.parametrize("dim", (1, 3, 5))
def test_oracle_against_brute_force_projector(dim):
    x, logits, gt = tiny()
    rng = np.random.default_rng(1)
    w, b = rng.standard_normal((3, 6)), rng.standard_normal(3)
    o = O.logit_origin(w, b)
    assert np.allclose(w @ o + b, 0.0, atol=1e-12)          # the origin maps to zero logits (C < F: the system is consistent)
    fit = O.Fit(x, logits, gt, o, dim)
    keep = gt >= 0
    a = x[keep].astype(np.float64) - o
    lam, vec = np.linalg.eigh(a.T @ a)
    top = vec[:, np.argsort(-lam)[:dim]]                    # the principal subspace, columns
    proj = np.eye(6) - top @ top.T                          # the explicit projector onto its complement
    norm = lambda rows: np.linalg.norm((rows.astype(np.float64) - o) @ proj, axis=1)
    alpha = logits[keep].astype(np.float64).max(axis=1).sum() / norm(x[keep]).sum()
    assert fit.count == int(keep.sum()) and np.isclose(fit.alpha, alpha, rtol=1e-10)
    assert np.allclose(fit.residual_norm(x), norm(x), rtol=1e-9, atol=1e-12)
    lg = logits.astype(np.float64)
    lse = np.log(np.exp(lg).sum(axis=1))
    assert np.allclose(fit.unknown_score(x, logits), alpha * norm(x) - lse, rtol=1e-9, atol=1e-10)
    e = np.exp(np.concatenate([lg, (alpha * norm(x))[:, None]], axis=1))
    p = fit.probabilities(x, logits)
    assert p.shape == (len(x), 4) and np.allclose(p, e / e.sum(axis=1, keepdims=True), rtol=1e-9, atol=1e-12)
    assert np.allclose(p.sum(axis=1), 1.0) and np.all(np.diff(fit.eigenvalues) <= 0)
    assert np.allclose(fit.components @ fit.S @ fit.components.T, np.diag(fit.eigenvalues), atol=1e-9 * fit.eigenvalues[0])


def test_oracle_scores_edge_cases():
    z = np.array([[3.0, 4.0], [0.0, 0.0], [NAN, 1.0]])
    lg = np.array([[0.0, 0.0], [-INF, -INF], [1.0, 2.0]], dtype=np.float32)
    assert O.scores(z, None, 0.0, O.NORM)[:2].tolist() == [5.0, 0.0] and np.isnan(O.scores(z, None, 0.0, O.NORM)[2])
    u = O.scores(z, lg, 2.0, O.UNKNOWN)
    assert u[0] == 10.0 - np.log(2.0) and u[1] == INF and np.isnan(u[2])
    p = O.scores(z, lg, 2.0, O.PROBS)
    assert np.allclose(p[0], np.array([1.0, 1.0, np.exp(10.0)]) / (2.0 + np.exp(10.0))) and p[1].tolist() == [0.0, 0.0, 1.0]
    assert np.isnan(p[2]).all()
    assert (O.default_dim(2048), O.default_dim(2047), O.default_dim(768), O.default_dim(767), O.default_dim(7)) == (1000, 512, 512, 383, 3)


def test_round_robin_pairs_are_disjoint_and_cover_every_pair_once():
    for F in (1, 2, 3, 4, 7, 8, 33):
        seen = set()
        assert O.rounds_of(F) == (F - 1 if F % 2 == 0 else F)
        for r in range(O.rounds_of(F)):
            k, p, q = O.partners(F, r)
            assert len(p) == F // 2 and (p < q).all() and np.array_equal(k[k], np.arange(F))
            assert len(set(p) | set(q)) == 2 * len(p) and (k == np.arange(F)).sum() == F % 2
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == F * (F - 1) // 2


# sweeps of the numpy restatement on the inputs of the GPU tests. The inputs come through LAPACK's QR and a BLAS product, whose last bits
# may differ between library builds, so a count may move by one; the GPU tests bound their errors with the device's own count.
SWEEPS = {("planted", 1): 1, ("planted", 2): 2, ("planted", 3): 4, ("planted", 15): 9, ("planted", 16): 8, ("planted", 17): 8,
          ("planted", 63): 11, ("planted", 64): 12, ("planted", 65): 11, ("planted", 130): 13, ("planted", 131): 13, ("planted", 515): 14,
          ("zeros", 33): 1, ("identity", 33): 1, ("ones", 33): 2, ("diag_ascending", 33): 1, ("repeated", 33): 12, ("rank_deficient", 33): 9}


@pytest.mark.parametrize("case", O.EIGH_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_numpy_jacobi_converges_on_the_inputs_of_the_gpu_tests(case):
    name, F = case
    S = O.eigh_input(name, F)
    assert np.array_equal(S, S.T)
    big = F > 200                                         # the count alone: the vectors are a third of the work
    w, v, sweeps = O.jacobi(S, vectors=not big)
    assert sweeps is not None and sweeps <= O.MAX_SWEEPS, "not converged"
    assert abs(sweeps - SWEEPS[case]) <= 1, sweeps
    scale = np.linalg.norm(S)
    want = O.eigh(S)[0]
    assert np.abs(w - want).max() <= 2 * O.eigh_error(F, sweeps) * scale
    if not big:
        assert np.linalg.norm(S @ v.T - v.T * w) <= O.eigh_error(F, sweeps) * scale
        assert np.linalg.norm(v @ v.T - np.eye(F)) <= O.orth_error(F, sweeps)


def test_end_to_end_input_has_its_gap_and_converges():
    x, logits, gt, weight, bias = O.e2e_data()
    fit = O.Fit(x, logits, gt, O.logit_origin(weight, bias), O.E2E_DIM)
    lam = fit.eigenvalues
    assert lam[O.E2E_DIM - 1] - lam[O.E2E_DIM] >= 0.02 * np.linalg.norm(fit.S)
    assert lam[O.E2E_DIM - 1] / lam[O.E2E_DIM] >= 1.26 and np.abs(fit.origin).max() > 0.1
    sweeps = O.jacobi(fit.S)[2]
    assert sweeps is not None and abs(sweeps - 12) <= 1, sweeps
    assert O.jacobi(fit.S, max_sweeps=1)[2] is None
    assert O.jacobi(O.eigh_input("planted", 17), max_sweeps=2)[2] is None
    # the other fits of the GPU test: every row counted, the zero origin, row 7 left out
    without7 = np.where(np.arange(len(gt)) == 7, -1, gt)
    for labels, origin in ((None, fit.origin), (gt, None), (without7, None)):
        other = O.Fit(x, logits, labels, origin, O.E2E_DIM)
        assert other.eigenvalues[O.E2E_DIM - 1] - other.eigenvalues[O.E2E_DIM] >= 0.02 * np.linalg.norm(other.S)
        sweeps = O.jacobi(other.S, vectors=False)[2]
        assert sweeps is not None and abs(sweeps - 12) <= 1, sweeps


# ------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("osi_vim_workspace", "osi_eigh_begin", "osi_eigh_sweep", "osi_eigh_finish", "osi_vim_project_f32", "osi_vim_scores")


def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 26
    for name in NAMES:
        assert hasattr(lib, name) and name in N.declared_symbols()
    assert (N.VIM_NORM, N.VIM_UNKNOWN, N.VIM_PROBS) == (O.NORM, O.UNKNOWN, O.PROBS) == (0, 1, 2)
    assert N.EIGH_MAX_F == O.MAX_F == 4096
    ops = N.ops()
    for name in ("eigh_begin", "eigh_sweep", "eigh_finish", "vim_project", "vim_scores"):
        assert hasattr(ops, name)


def test_abi_entries_validate_before_launch():
    """Each null required pointer (logits may be NULL for OSI_VIM_NORM), a size <= 0, sizes past the limits, a bad enum, an alpha that
    is not finite, both or neither output of the scores, a workspace one byte short, absent or misaligned: OSI_ERR_ARG, nothing
    launched (safe on a CPU-only host; the pointers are never dereferenced on the host)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    for args in ((0, 4, 5), (100, 0, 5), (100, 4, 0), (-1, 4, 5), (100, -2, 5), (100, 4, -7), (100, 4, N.EIGH_MAX_F + 1),
                 (100, N.EIGH_MAX_F + 1, 40)):
        assert lib.osi_vim_workspace(*args) == 0, args
    nb = lib.osi_vim_workspace(100, 4, 40)
    assert nb > 64 + 16 * 40 and nb % 8 == 0 and lib.osi_vim_workspace(1, 1, 40) == nb and lib.osi_vim_workspace(1, 1, 41) % 8 == 0
    assert lib.osi_vim_workspace(1, 1, N.EIGH_MAX_F) > nb
    p = 4096                                             # any non-null, aligned address: argument checks come first

    def refuses(fn, good, pointers, values):
        for hole in pointers:
            args = list(good); args[hole] = None
            assert fn(*args) == -1, (fn.__name__, hole)
        for pos, value in values:
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (fn.__name__, pos, value)

    sizes = lambda pos: ((pos, 0), (pos, -1), (pos, N.EIGH_MAX_F + 1))
    refuses(lib.osi_eigh_begin, [p, 40, p, p, p, p, p, nb, None], (0, 2, 3, 4, 5, 6), sizes(1) + ((7, nb - 1), (7, 64), (7, 0), (6, p + 4)))
    refuses(lib.osi_eigh_sweep, [p, p, 40, p, p, p, p, nb, None], (0, 1, 3, 4, 5, 6), sizes(2) + ((7, nb - 1), (7, 64), (7, 0), (6, p + 4)))
    refuses(lib.osi_eigh_finish, [p, p, 40, p, p, p, p, nb, None], (0, 1, 3, 4, 5, 6), sizes(2) + ((7, nb - 1), (7, 0), (6, p + 4)))
    big = 1 << 20                                        # big * 2048 = 2^31 elements: one past the limit
    refuses(lib.osi_vim_project_f32, [p, p, 100, 40, p, 7, p, p, nb, None], (0, 1, 4, 6, 7),
            ((2, 0), (2, -1)) + sizes(3) + sizes(5) + ((8, 63), (8, 0), (7, p + 4)))
    assert lib.osi_vim_project_f32(p, p, big, 2048, p, 7, p, p, 1 << 40, None) == -1
    assert lib.osi_vim_project_f32(p, p, big, 8, p, 2048, p, p, 1 << 40, None) == -1          # M * K = 2^31
    good = [p, 100, 7, p, 4, 1.5, N.VIM_PROBS, p, None, p, nb, None]
    refuses(lib.osi_vim_scores, good, (0, 3, 7, 9),
            ((1, 0), (1, -1)) + sizes(2) + ((4, 0), (4, -1), (5, NAN), (5, INF), (5, -INF), (6, 3), (6, -1), (8, p), (10, 63), (10, 0), (9, p + 4)))
    f64 = list(good); f64[7] = None; f64[8] = p            # the fp64 output alone is fine as far as the checks go: only sizes can refuse it
    bad = list(f64); bad[1] = 0
    assert lib.osi_vim_scores(*bad) == -1
    assert lib.osi_vim_scores(p, big, 2048, p, 4, 1.0, N.VIM_UNKNOWN, p, None, p, 1 << 40, None) == -1        # M * K = 2^31
    assert lib.osi_vim_scores(p, 1 << 16, 8, p, (1 << 15) - 1, 1.0, N.VIM_PROBS, p, None, p, 1 << 40, None) == -1   # M * (C + 1) = 2^31
    norm = [p, 100, 7, None, 0, NAN, N.VIM_NORM, p, None, p, nb, None]                          # NORM reads neither logits nor alpha
    for pos, value in ((0, None), (7, None), (1, 0), (2, 0), (10, 63)):
        args = list(norm); args[pos] = value
        assert lib.osi_vim_scores(*args) == -1, (pos, value)


# ---------------------------------------------------------------------------------------------------------------- Python
def hand_state(f=4, dim=2, classes=3):
    return dict(origin=torch.arange(f, dtype=torch.float64), eigenvalues=torch.arange(f, 0, -1).double(),
                components=torch.eye(f, dtype=torch.float64).flip(0).contiguous(), dim=dim, alpha=0.75, count=10, classes=classes)


def test_names_import_and_refuse_without_gpu():
    import openset_imagenet
    from openset_imagenet.vim import ViM, eigh
    from openset_imagenet.script.evaluate import vim_arrays
    assert openset_imagenet.ViM is ViM and "ViM" in openset_imagenet.__all__
    x, logits, gt = tiny()
    x4 = x[:, :4]
    vim = ViM(dim=2)
    loaded = ViM().load_state_dict(hand_state())
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert vim.fit(x, logits, gt).predict(x, logits).shape == (len(x), 3) and loaded.residual_norm(x4).shape == (len(x),)
    else:
        train = dict(gt=gt, logits=logits, features=x)
        for call in (lambda: vim.fit(x, logits, gt), lambda: loaded.predict(x4, logits), lambda: loaded.residual_norm(x4),
                     lambda: loaded.unknown_score(x4, logits), lambda: loaded.probabilities(x4, logits), lambda: eigh(np.eye(3)),
                     lambda: vim_arrays(train, train, 2)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()


def test_host_side_checks_name_the_argument():
    from openset_imagenet.vim import ViM, eigh
    for bad in (0, -3):
        with pytest.raises(ValueError, match="dim must"):
            ViM(dim=bad)
    for bad in ("2", 2.0, True):
        with pytest.raises(TypeError, match="dim must"):
            ViM(dim=bad)
    for bad in ("mean", "", np.zeros((2, 2)), []):
        with pytest.raises(ValueError, match="origin must"):
            ViM(origin=bad)
    for bad in (None, 0.0, 1, False):
        with pytest.raises(TypeError, match="origin must"):
            ViM(origin=bad)
    m = ViM(dim=3, origin=[1, 2, 3, 4, 5, 6])
    assert m.requested_dim == 3 and m.requested_origin.dtype == torch.float64 and not m.is_fitted
    x, logits, gt = tiny()
    for call, what in ((lambda: m.predict(x, logits), "predict"), (lambda: m.residual_norm(x), "residual_norm"),
                       (lambda: m.unknown_score(x, logits), "unknown_score"), (lambda: m.probabilities(x, logits), "probabilities"),
                       (lambda: m.state_dict(), "state_dict")):
        with pytest.raises(ValueError, match=f"{what} before fit"):
            call()
    # shape checks come before any GPU work: they raise ValueError on a host without a GPU too
    with pytest.raises(ValueError, match="features must be a matrix"):
        m.fit(x[0], logits[:1])
    with pytest.raises(ValueError, match="logits must be a matrix"):
        m.fit(x, logits[:-1])
    with pytest.raises(ValueError, match="disagree on the number of samples"):
        m.fit(x, logits, gt[:-1])
    with pytest.raises(ValueError, match="must not be empty"):
        m.fit(x[:0], logits[:0])
    with pytest.raises(ValueError, match="chunk must"):
        m.fit(x, logits, gt, chunk=0)
    with pytest.raises(ValueError, match="at most 4096"):
        m.fit(np.zeros((2, 4097), dtype=np.float32), logits[:2])
    for dim in (6, 7):
        with pytest.raises(ValueError, match="0 < dim < F"):
            ViM(dim=dim).fit(x, logits, gt)
    with pytest.raises(ValueError, match="0 < dim < F"):
        ViM().fit(x[:, :1], logits, gt)                   # F // 2 = 0
    with pytest.raises(ValueError, match="origin holds 6 values"):
        m.fit(x[:, :5], logits, gt)
    with pytest.raises(ValueError, match="weight is needed"):
        ViM(dim=2).fit(x, logits, gt, bias=np.zeros(3))
    with pytest.raises(ValueError, match=r"weight must be \[3, 6\]"):
        ViM(dim=2).fit(x, logits, gt, weight=np.zeros((6, 3)), bias=np.zeros(3))
    with pytest.raises(ValueError, match=r"bias must be \[3\]"):
        ViM(dim=2).fit(x, logits, gt, weight=np.zeros((3, 6)), bias=np.zeros(4))
    with pytest.raises(ValueError, match="must be finite"):
        ViM(dim=2).fit(x, logits, gt, weight=np.full((3, 6), NAN), bias=np.zeros(3))
    loaded = ViM().load_state_dict(hand_state())
    with pytest.raises(ValueError, match=r"features must be \[M, 4\]"):
        loaded.residual_norm(x)
    with pytest.raises(ValueError, match=r"logits must be \[50, 3\]"):
        loaded.unknown_score(x[:, :4], logits[:, :2])
    with pytest.raises(ValueError, match="chunk must"):
        loaded.probabilities(x[:, :4], logits, chunk=-2)
    with pytest.raises(ValueError, match="square matrix"):
        eigh(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="at most 4096"):
        eigh(torch.zeros(4097, 4097, dtype=torch.int8))
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_sweeps must"):
            eigh(np.eye(3), max_sweeps=bad)


def test_state_dict_bookkeeping():
    from openset_imagenet.vim import ViM
    sd = hand_state()
    m = ViM().load_state_dict(sd)
    assert m.is_fitted and (m.dim, m.alpha, m.count, m.classes) == (2, 0.75, 10, 3)
    assert m.components.dtype == torch.float64 and m.components.device.type == "cpu"
    back = m.state_dict()
    assert set(back) == set(sd)
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(back[k], v) and back[k].data_ptr() != getattr(m, k).data_ptr()     # copies, not views
        else:
            assert back[k] == v, k
    again = ViM(dim=1).load_state_dict(back)
    assert again.dim == 2 and torch.equal(again.components, m.components)
    for drop in ("components", "alpha", "classes"):
        with pytest.raises(ValueError, match="lacks"):
            ViM().load_state_dict({k: v for k, v in sd.items() if k != drop})
    with pytest.raises(ValueError, match=r"components must be \[F, F\]"):
        ViM().load_state_dict(dict(sd, components=torch.zeros(4, 3)))
    with pytest.raises(ValueError, match="origin must have shape"):
        ViM().load_state_dict(dict(sd, origin=torch.zeros(3)))
    with pytest.raises(ValueError, match="eigenvalues must have shape"):
        ViM().load_state_dict(dict(sd, eigenvalues=torch.zeros(5)))
    with pytest.raises(ValueError, match="0 < dim < F"):
        ViM().load_state_dict(dict(sd, dim=4))
    with pytest.raises(ValueError, match="alpha must be finite"):
        ViM().load_state_dict(dict(sd, alpha=NAN))
    with pytest.raises(ValueError, match="classes must be positive"):
        ViM().load_state_dict(dict(sd, classes=0))


def test_evaluate_takes_and_refuses_the_options():
    from openset_imagenet.script.evaluate import get_args
    a = get_args(["entropic", "2"])
    assert a.vim is False and a.vim_dim is None
    a = get_args(["softmax", "1", "--vim", "--vim-dim", "256", "--mahalanobis"])
    assert a.vim is True and a.vim_dim == 256 and a.mahalanobis is True
    for bad in (["garbage", "1", "--vim"], ["softmax", "1", "--vim", "--vim-dim", "0"], ["softmax", "1", "--vim-dim", "-4"],
                ["softmax", "1", "--vim-dim", "1.5"]):
        with pytest.raises(SystemExit):
            get_args(bad)

"""GPU parity of ViM and its eigensolver (csrc/vim.hip, openset_imagenet/vim.py) against the numpy fp64 oracle of tests/vim_oracle.py:
every call through the C ABI on identical input bits, with 256-byte guard bands around every output and a fresh workspace full of 0xFF
bytes for every call, then the whole of ViM.fit and the scoring calls.

Every bound is derived, none measured; u = 2^-53, gamma_k = k u / (1 - k u), s = the sweeps the device ran, r = 2 s (F - 1) rotation
stages on A:
  eigensolver   one rotation applied to a 2-vector has error <= 10 u of its norm (6 u from the two products and the sum with computed c
                and s, 4 u from forming c and s), so |S V - V L|_F <= (10 r u + F 2^-52) |S|_F (the second term is the off-diagonal mass
                the threshold 2^-52 |S|_F leaves) and |V V^T - I|_F <= 20 s (F - 1) u sqrt(F). The sorted values of a nearly orthogonal V
                with residual R are within |R| / sigma_min(V) of the true ones (Kahan), sigma_min(V)^2 >= 1 - |V^T V - I|; np.linalg.eigh is
                held to its own measured residual in the same way. Values sorted, the sign rule, a second run equal bits.
  project       |z - (x - o) R^T| <= 2 gamma_F |x - o| |R|^T on the device's own R.
  scores        fp32 outputs within one fp32 ulp of the oracle applied to the device's z; fp64 outputs: the norm within 2 gamma_{K+2} n
                (both sides sum K squares and take one root), the unknown score within 2 gamma_{K+4} |alpha n| + 2 gamma_{C+8} (1 +
                |lse|) + 4 u |result| (the exponentials and the logarithm round a few times each; a relative error of the sum is an
                absolute one of its logarithm), a probability p within p (4 gamma_{K+4} |alpha n| + 2 gamma_{C+10}); rows of the fp32
                probabilities sum to 1 within C 2^-23.
  end to end    F = 96 with a planted gap at dim: (lambda_dim - lambda_dim+1) >= 0.02 |S|_F is asserted on the oracle. By Davis-Kahan the
                residual projector moves by at most 2 eps / 0.02 for a perturbation eps |S|_F; both sides carry one (the device's bounded
                by eps(F, 30), the oracle's far below), so a residual norm may differ by 4 eps(F, 30) / 0.02 |x - o| plus one fp32 ulp."""
import numpy as np
import pytest
import torch

import vim_oracle as O
from gpu_harness import Out, call, on, poisoned, ulp32

pytestmark = pytest.mark.gpu

MS, KS, CS = (1, 5, 63, 257), (1, 16, 65), (1, 7)


# --------------------------------------------------------------------------------------------------------------- helpers
def workspace(M, K, F, cuda):
    from openset_imagenet import _native as NL
    nb = NL.lib().osi_vim_workspace(M, K, F)
    return poisoned(nb, cuda), nb


def run_eigh(cuda, S, max_sweeps=O.MAX_SWEEPS):
    """begin, sweeps until one rotates nothing, finish. Returns values, vectors (rows), head, info, the rotations of every sweep."""
    from openset_imagenet import _native as NL
    lib, F = NL.lib(), len(S)
    A, Vt = Out((F, F), torch.float64, cuda), Out((F, F), torch.float64, cuda)
    head, info, rot = Out((2,), torch.float64, cuda), Out((1,), torch.int32, cuda), Out((1,), torch.int64, cuda)
    ws, nb = workspace(1, 1, F, cuda)
    call(lib.osi_eigh_begin, *on(cuda, S), F, A, Vt, head, info, ws, nb)
    rotations = []
    for _ in range(max_sweeps):
        ws, nb = workspace(1, 1, F, cuda)
        call(lib.osi_eigh_sweep, A, Vt, F, head, info, rot, ws, nb)
        rotations.append(int(rot.np()[0]))
        if rotations[-1] == 0:
            break
    evals, evecs = Out((F,), torch.float64, cuda), Out((F, F), torch.float64, cuda)
    ws, nb = workspace(1, 1, F, cuda)
    call(lib.osi_eigh_finish, A, Vt, F, info, evals, evecs, ws, nb)
    for o in (A, Vt, head, info, rot, evals, evecs):
        assert o.check()
    return evals.np(), evecs.np(), head.np(), int(info.np()[0]), rotations


def run_project(cuda, x, origin, R):
    from openset_imagenet import _native as NL
    (M, F), K = x.shape, len(R)
    ws, nb = workspace(M, K, F, cuda)
    z = Out((M, K), torch.float64, cuda)
    call(NL.lib().osi_vim_project_f32, *on(cuda, x), *on(cuda, origin), M, F, *on(cuda, R), K, z, ws, nb)
    assert z.check()
    return z.np()


def run_scores(cuda, z, logits, alpha, mode, f64=False):
    from openset_imagenet import _native as NL
    M, K = z.shape
    C = 1 if logits is None else logits.shape[1]
    ws, nb = workspace(M, K, K, cuda)
    out = Out((M, C + 1) if mode == O.PROBS else (M,), torch.float64 if f64 else torch.float32, cuda)
    call(NL.lib().osi_vim_scores, *on(cuda, z), M, K, *on(cuda, logits), C, float(alpha), mode, None if f64 else out, out if f64 else None,
         ws, nb)
    assert out.check()
    return out.np()


def check_decomposition(S, w, v, sweeps):
    """The derived bounds of a converged solve; returns nothing."""
    F, scale = len(S), np.linalg.norm(S)
    eps, orth = O.eigh_error(F, sweeps), O.orth_error(F, sweeps)
    assert np.linalg.norm(S @ v.T - v.T * w) <= eps * scale, "residual"
    assert np.linalg.norm(v @ v.T - np.eye(F)) <= orth, "orthogonality"
    assert (np.diff(w) <= 0).all(), "sorted"
    assert np.array_equal(v, O.signed(v)), "sign rule"
    we, ve = O.eigh(S)
    own = np.linalg.norm(S @ ve.T - ve.T * we) / np.sqrt(max(1.0 - np.linalg.norm(ve @ ve.T - np.eye(F)), 0.5))
    assert np.abs(w - we).max() <= eps * scale / np.sqrt(1.0 - orth) + own, "values"


# ------------------------------------------------------------------------------------------------------------ eigensolver
@pytest.mark.parametrize("F", O.PLANTED_F)
def test_eigh_on_second_moments_of_planted_rows(cuda, F):
    S = O.eigh_input("planted", F)
    w, v, head, info, rotations = run_eigh(cuda, S)
    assert info == 0 and rotations[-1] == 0 and len(rotations) <= O.MAX_SWEEPS, rotations
    scale = np.linalg.norm(S)
    assert abs(head[0] - scale) <= O.gamma(F * F + 2) * scale and head[1] == head[0] * 2.0 ** -52
    check_decomposition(S, w, v, len(rotations))
    w2, v2, head2, _, rotations2 = run_eigh(cuda, S)
    assert np.array_equal(w2, w) and np.array_equal(v2, v) and np.array_equal(head2, head) and rotations2 == rotations, "a second run"


def test_eigh_special_matrices(cuda):
    F = O.SPECIAL_F
    eye = np.eye(F)
    for name, values in (("zeros", np.zeros(F)), ("identity", np.ones(F))):
        w, v, head, info, rotations = run_eigh(cuda, O.eigh_input(name, F))
        assert info == 0 and rotations == [0] and np.array_equal(w, values) and np.array_equal(v, eye), name
    assert head[0] == np.sqrt(float(F))
    S = O.eigh_input("diag_ascending", F)                  # the sort and the row permutation
    w, v, _, info, rotations = run_eigh(cuda, S)
    assert info == 0 and rotations == [0] and np.array_equal(w, np.arange(float(F), 0.0, -1.0)) and np.array_equal(v, eye[::-1])
    S = O.eigh_input("ones", F)                            # rank 1, lambda_1 = F
    w, v, _, info, rotations = run_eigh(cuda, S)
    assert info == 0 and rotations[-1] == 0
    check_decomposition(S, w, v, len(rotations))
    eps = O.eigh_error(F, len(rotations)) * F
    assert abs(w[0] - F) <= eps and np.abs(w[1:]).max() <= eps and np.abs(v[0] - 1 / np.sqrt(F)).max() <= 4 * eps
    for name in ("repeated", "rank_deficient"):
        S = O.eigh_input(name, F)
        w, v, _, info, rotations = run_eigh(cuda, S)
        assert info == 0 and rotations[-1] == 0 and len(rotations) <= O.MAX_SWEEPS, (name, rotations)
        check_decomposition(S, w, v, len(rotations))
    assert np.abs(w[F // 2:]).max() <= O.eigh_error(F, len(rotations)) * np.linalg.norm(S)           # F // 2 rows: that rank at most


@pytest.mark.parametrize("bad", (np.nan, np.inf))
def test_eigh_refuses_a_matrix_that_is_not_finite(cuda, bad):
    S = O.eigh_input("planted", 17)
    S[3, 11] = S[11, 3] = bad
    w, v, head, info, rotations = run_eigh(cuda, S, max_sweeps=2)
    assert info == 1 and rotations == [0] and np.isnan(w).all() and not v.any() and not np.isfinite(head[0])


# ----------------------------------------------------------------------------------------------------- project and scores
_BASIS = {}


def device_basis(cuda, F=131):
    """Eigenvectors of the planted second moment from the device itself, once, shared and left unchanged."""
    if F not in _BASIS:
        w, v, _, info, _ = run_eigh(cuda, O.eigh_input("planted", F))
        assert info == 0
        v.setflags(write=False)
        _BASIS[F] = v
    return _BASIS[F]


def score_bounds(z, logits, alpha):
    K, C = z.shape[1], logits.shape[1]
    n = O.scores(z, None, 0.0, O.NORM)
    v = np.abs(alpha * n)
    lse = O.logsumexp(logits)
    unknown = O.scores(z, logits, alpha, O.UNKNOWN)
    probs = O.scores(z, logits, alpha, O.PROBS)
    return (2 * O.gamma(K + 2) * n, 2 * O.gamma(K + 4) * v + 2 * O.gamma(C + 8) * (1 + np.abs(lse)) + 4 * O.U * np.abs(unknown),
            probs * (4 * O.gamma(K + 4) * v + 2 * O.gamma(C + 10))[:, None])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_project_and_scores(cuda, M, K):
    F = 131
    R = device_basis(cuda)[F - K:]
    rng = np.random.default_rng(300 + 7 * M + K)
    x = (O.planted_rows(F, M, np.geomspace(2.0, 0.05, F), 500 + M) + 0.3).astype(np.float32)
    origin = 0.2 * rng.standard_normal(F)
    z = run_project(cuda, x, origin, R)
    a = np.abs(x.astype(np.float64) - origin)
    assert (np.abs(z - O.project(x, origin, R)) <= 2 * O.gamma(F) * (a @ np.abs(R).T)).all(), "project"
    assert np.array_equal(run_project(cuda, x, origin, R), z), "a second call"
    for C in CS:
        logits = (3 * rng.standard_normal((M, C))).astype(np.float32)
        alpha = float(np.abs(logits).max() / max(np.sqrt((z * z).sum(axis=1)).mean(), 1e-3))
        bounds = score_bounds(z, logits, alpha)
        for mode, bound in zip((O.NORM, O.UNKNOWN, O.PROBS), bounds):
            want = O.scores(z, logits, alpha, mode)
            got64 = run_scores(cuda, z, logits, alpha, mode, True)
            got32 = run_scores(cuda, z, logits, alpha, mode)
            assert got64.shape == got32.shape == want.shape and got32.dtype == np.float32
            assert (np.abs(got64 - want) <= bound).all(), (C, mode, "fp64")
            assert (np.abs(got32.astype(np.float64) - want) <= ulp32(want)).all(), (C, mode, "fp32")
            assert np.array_equal(got32, got64.astype(np.float32)), (C, mode, "rounded once")
        probs = run_scores(cuda, z, logits, alpha, O.PROBS)
        assert (np.abs(probs.astype(np.float64).sum(axis=1) - 1.0) <= C * 2.0 ** -23).all()
    assert np.array_equal(run_scores(cuda, z, None, 0.0, O.NORM, True), run_scores(cuda, z, logits, alpha, O.NORM, True))


def test_scores_propagate_nan(cuda):
    rng = np.random.default_rng(3)
    M, K, C = 9, 65, 7
    z, logits = rng.standard_normal((M, K)), rng.standard_normal((M, C)).astype(np.float32)
    z[2, 64] = np.nan
    logits[5, 6] = np.nan
    for f64 in (False, True):
        n = run_scores(cuda, z, logits, 1.5, O.NORM, f64)
        assert np.array_equal(np.isnan(n), np.arange(M) == 2)
        u = run_scores(cuda, z, logits, 1.5, O.UNKNOWN, f64)
        assert np.array_equal(np.isnan(u), np.isin(np.arange(M), (2, 5)))
        p = run_scores(cuda, z, logits, 1.5, O.PROBS, f64)
        assert np.array_equal(np.isnan(p), np.isin(np.arange(M), (2, 5))[:, None] & np.ones((1, C + 1), dtype=bool))


# -------------------------------------------------------------------------------------------------------------- end to end
def test_fit_and_scores_end_to_end(cuda):
    from openset_imagenet import ViM
    from openset_imagenet.script.evaluate import vim_arrays
    F, dim, C = O.E2E_F, O.E2E_DIM, O.E2E_C
    x, logits, gt, weight, bias = O.e2e_data()
    ref = O.Fit(x, logits, gt, O.logit_origin(weight, bias), dim)
    scale = np.linalg.norm(ref.S)
    assert ref.eigenvalues[dim - 1] - ref.eigenvalues[dim] >= 0.02 * scale
    vim = ViM(dim=dim).fit(x, torch.tensor(logits), torch.tensor(gt), weight=weight, bias=torch.tensor(bias))
    assert vim.count == ref.count == int((gt >= 0).sum()) and vim.classes == C and vim.dim == dim and 1 <= vim.sweeps <= 30
    assert vim.components.dtype == vim.eigenvalues.dtype == vim.origin.dtype == torch.float64 and vim.components.is_cuda
    assert np.array_equal(vim.origin.cpu().numpy(), ref.origin) and np.abs(ref.origin).max() > 0.1
    eps = O.eigh_error(F, 30)
    assert np.abs(vim.eigenvalues.cpu().numpy() - ref.eigenvalues).max() <= 2 * (eps + 2 * O.gamma(len(x))) * scale
    q, ql, _, _, _ = O.e2e_data(seed=33, n=203)
    dist = np.linalg.norm(q.astype(np.float64) - ref.origin, axis=1)
    slack = 4 * eps / 0.02 * dist                          # Davis-Kahan, both sides
    want_n = ref.residual_norm(q)
    norm = vim.residual_norm(q)
    assert norm.dtype == torch.float32 and norm.is_cuda and norm.shape == (203,)
    assert (np.abs(norm.cpu().numpy().astype(np.float64) - want_n) <= slack + ulp32(want_n)).all()
    # alpha = sum of the largest logits / sum of the norms: the norms of the training rows carry the same slack, the sums gamma_N each
    train_slack = (4 * eps / 0.02 * np.linalg.norm(x[gt >= 0].astype(np.float64) - ref.origin, axis=1)).sum()
    d_alpha = abs(ref.alpha) * (train_slack / ref.residual_norm(x[gt >= 0]).sum() + 4 * O.gamma(len(x)))
    assert abs(vim.alpha - ref.alpha) <= d_alpha
    d_virtual = abs(ref.alpha) * slack + d_alpha * want_n   # of the virtual logit alpha n
    unknown, probs, pred = vim.unknown_score(q, ql), vim.probabilities(torch.tensor(q), ql), vim.predict(q, torch.tensor(ql))
    want_u, want_p = ref.unknown_score(q, ql), ref.probabilities(q, ql)
    assert unknown.shape == (203,) and probs.shape == (203, C + 1) and pred.shape == (203, C) and probs.dtype == torch.float32
    assert (np.abs(unknown.cpu().numpy().astype(np.float64) - want_u) <= d_virtual + ulp32(want_u)).all()
    # |d softmax / d virtual logit| <= 1 / 4 on every column
    assert (np.abs(probs.cpu().numpy().astype(np.float64) - want_p) <= 0.25 * d_virtual[:, None] + ulp32(want_p)).all()
    assert torch.equal(pred, probs[:, :C])
    # chunked = unchunked, bit for bit; on the device as well as from the host
    assert torch.equal(vim.residual_norm(q, chunk=64), norm) and torch.equal(vim.unknown_score(torch.tensor(q).cuda(), ql, chunk=5), unknown)
    assert torch.equal(vim.probabilities(q, torch.tensor(ql).cuda(), chunk=100), probs)
    # a chunked fit: the scatter accumulates row chunks; the same bounds hold
    chunked = ViM(dim=dim).fit(x, logits, gt, weight=weight, bias=bias, chunk=250)
    assert abs(chunked.alpha - ref.alpha) <= d_alpha
    assert (np.abs(chunked.residual_norm(q).cpu().numpy().astype(np.float64) - want_n) <= slack + ulp32(want_n)).all()
    # an explicit origin is taken as it is; gt = None counts every row
    explicit = ViM(dim=dim, origin=ref.origin).fit(x, logits)
    assert explicit.count == len(x) and np.array_equal(explicit.origin.cpu().numpy(), ref.origin)
    # the state dict round-trips: host tensors, moved on first use, the same bits out
    sd = vim.state_dict()
    assert all(not isinstance(v, torch.Tensor) or v.device.type == "cpu" for v in sd.values())
    again = ViM().load_state_dict(sd)
    assert again.components.device.type == "cpu" and again.alpha == vim.alpha
    assert torch.equal(again.unknown_score(q, ql), unknown) and again.components.is_cuda and torch.equal(again.probabilities(q, ql), probs)
    # evaluate.py's helper: zero origin (a network without a logit bias), fitted once, taken as it is afterwards
    train, split = dict(gt=gt, logits=logits, features=x), dict(gt=np.zeros(203, dtype=np.int64), logits=ql, features=q)
    fitted, arrays = vim_arrays(train, split, dim)
    zero = O.Fit(x, logits, gt, None, dim)
    assert not fitted.origin.any() and set(arrays) == {"gt", "logits", "features", "scores", "unknown"}
    assert arrays["scores"].shape == (203, C) and arrays["unknown"].shape == (203,)
    z_slack = 4 * eps / 0.02 * np.linalg.norm(q.astype(np.float64), axis=1)
    assert (np.abs(fitted.residual_norm(q).cpu().numpy() - zero.residual_norm(q)) <= z_slack + ulp32(zero.residual_norm(q))).all()
    assert np.array_equal(vim_arrays(fitted, split)[1]["unknown"], arrays["unknown"])


def test_fit_raises_without_convergence_and_on_nan(cuda):
    from openset_imagenet import ViM
    from openset_imagenet.vim import eigh
    x, logits, gt, _, _ = O.e2e_data()
    hasty = ViM(dim=O.E2E_DIM)
    hasty.max_sweeps = 1
    with pytest.raises(ValueError, match="no eigen-decomposition.*not converged after 1 sweeps"):
        hasty.fit(x, logits, gt)
    assert not hasty.is_fitted
    bad = x.copy()
    bad[7, 3] = np.nan
    with pytest.raises(ValueError, match="no eigen-decomposition.*not finite"):
        ViM(dim=O.E2E_DIM).fit(bad, logits, np.where(np.arange(len(gt)) == 7, 0, gt))
    assert ViM(dim=O.E2E_DIM).fit(bad, logits, np.where(np.arange(len(gt)) == 7, -1, gt)).is_fitted     # an uncounted row is not read
    S = O.eigh_input("planted", 17)
    with pytest.raises(ValueError, match="not converged after 2 sweeps"):
        eigh(S, max_sweeps=2)
    w, v, sweeps = eigh(torch.tensor(S))
    assert w.is_cuda and v.shape == (17, 17) and sweeps <= 30
    check_decomposition(S, w.cpu().numpy(), v.cpu().numpy(), sweeps)

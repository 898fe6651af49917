"""GPU parity of the Mahalanobis scores (csrc/mahalanobis.hip, openset_imagenet/mahalanobis.py) against the numpy fp64 oracle of
tests/mahalanobis_oracle.py: every call through the C ABI on identical input bits, with 256-byte guard bands around every output and
a workspace full of 0xFF bytes, then the whole of Mahalanobis.fit / distances / predict / unknown_score.

Every bound is derived, none measured; u = 2^-53, gamma_k = k u / (1 - k u):
  means, scatter on integer inputs   |x| <= 64 and integer `mean` inputs: every product and sum is exact in fp64 in any order, the mean
                      is one IEEE division of an exact sum. EQUAL BITS with the oracle; S == S.T; a second call, permuted rows and two
                      `accumulate` halves change no bit.
  scatter, real       |S - S_ref| <= 2 gamma_n sum_k |a_ki| |a_kj|: both sides are within gamma_n of the exact sum of the same products.
  factor              with Sigma formed by the oracle from the device's own S: |L L^T - Sigma| <= 2 gamma_{F+8} |L| |L^T| (Higham, any
                      summation order; 2 for forming Sigma and its trace), |W L - I| <= 2 gamma_F |W| |L| (W is built by rows), strict
                      upper triangles exactly zero, logdet within gamma_{2F} sum |ln L_ii| of the sum over the device's own diagonal.
  whiten              |z - x W^T| <= 2 gamma_F |x| |W|^T on the device's own W.
  scores              Gaussian blobs, shrinkage 0.1, cond(Sigma) <= 1e4 asserted here on the CPU (F u cond <= 3e-9 even at F = 2048):
                      within one fp32 ulp of the reference, plus 1e-8 (d2_c + d2_0) for the relative form, whose subtraction cancels;
                      the arg-min class equal on EVERY row, the oracle's own gap between the two smallest distances above 1e-6 relative.
Shapes: F around the 16-wide MFMA tile, the 64-wide workgroup tile and the 64-column panel (63, 65, 131 = nb - 1, nb + 1, 2 nb + 3), N
around the K step of 4, the LDS stage of 16 and the row split, C in {1, 3, 7} with one empty class and labels -1 and C among the rows,
and one case at the workload's width (F = 2048, N = 4096)."""
import numpy as np
import pytest
import torch

import mahalanobis_oracle as O
from gpu_harness import Out, call, on, poisoned, ulp32

pytestmark = pytest.mark.gpu

FS = (1, 15, 16, 17, 63, 64, 65, 130, 131)
NS = (1, 3, 4, 5, 63, 257, 1031)
CS = (1, 3, 7)


# --------------------------------------------------------------------------------------------------------------- helpers
def workspace(N, C, F, cuda):
    from openset_imagenet import _native as NL
    nb = NL.lib().osi_maha_workspace(N, C, F)
    return poisoned(nb, cuda), nb


def run_means(cuda, x, gt, C):
    from openset_imagenet import _native as NL
    N, F = x.shape
    ws, nb = workspace(N, C, F, cuda)
    mean, count = Out((C + 1, F), torch.float64, cuda), Out((C + 1,), torch.int64, cuda)
    call(NL.lib().osi_maha_class_means, *on(cuda, x), *on(cuda, gt), N, C, F, mean, count, ws, nb)
    assert mean.check() and count.check()
    return mean.np(), count.np()


def run_scatter(cuda, x, gt, mean, C, mode, into=None):
    """S of one call; `into` (an Out) is accumulated into instead."""
    from openset_imagenet import _native as NL
    N, F = x.shape
    ws, nb = workspace(N, C, F, cuda)
    S = into if into is not None else Out((F, F), torch.float64, cuda)
    call(NL.lib().osi_maha_scatter, *on(cuda, x), *on(cuda, gt), *on(cuda, mean), N, C, F, mode, int(into is not None), S, ws, nb)
    assert S.check()
    return S


def run_factor(cuda, S, scale, shrinkage):
    from openset_imagenet import _native as NL
    F = len(S)
    ws, nb = workspace(1, 1, F, cuda)
    L, W = Out((F, F), torch.float64, cuda), Out((F, F), torch.float64, cuda)
    logdet, info = Out((1,), torch.float64, cuda), Out((1,), torch.int32, cuda)
    call(NL.lib().osi_maha_factor, *on(cuda, S), F, float(scale), float(shrinkage), L, W, logdet, info, ws, nb)
    assert L.check() and W.check() and logdet.check() and info.check()
    return L.np(), W.np(), float(logdet.np()[0]), int(info.np()[0])


def run_whiten(cuda, x, W):
    from openset_imagenet import _native as NL
    M, F = x.shape
    ws, nb = workspace(1, 1, F, cuda)
    z = Out((M, F), torch.float64, cuda)
    fn = NL.lib().osi_maha_whiten_f32 if x.dtype == np.float32 else NL.lib().osi_maha_whiten_f64
    call(fn, *on(cuda, x), M, F, *on(cuda, W), z, ws, nb)
    assert z.check()
    return z.np()


def run_sqdist(cuda, z, zm, minus=None, what=O.RAW, f64=False):
    from openset_imagenet import _native as NL
    (M, F), C = z.shape, len(zm)
    ws, nb = workspace(1, 1, F, cuda)
    out = Out((M, C), torch.float64 if f64 else torch.float32, cuda)
    call(NL.lib().osi_maha_sqdist, *on(cuda, z), M, *on(cuda, zm), C, F, *on(cuda, minus), what, None if f64 else out, out if f64 else None,
         ws, nb)
    assert out.check()
    return out.np()


def labels(rng, N, C):
    """Labels in [0, C) with class C - 2 empty when C > 2, and a -1, a -7 and a label C among the rows when there is room."""
    gt = rng.integers(0, C, N)
    if C > 2:
        gt[gt == C - 2] = C - 1
    if N >= 5:
        gt[1], gt[N // 2], gt[N - 1] = -1, C, -7
    return gt.astype(np.int64)


def blobs(seed, N, C, F, spread=3.0):
    """Gaussian blobs: unit-variance rows around well separated class centres; the labels of `labels`."""
    rng = np.random.default_rng(seed)
    gt = labels(rng, N, C)
    centres = spread * rng.standard_normal((C + 1, F))
    x = (rng.standard_normal((N, F)) + centres[np.clip(gt, 0, C)]).astype(np.float32)
    return x, gt


def mean_bound(x, gt, C):
    """2 gamma_n sum |x| / count: both sides are within gamma_n of the exact sum before the one division."""
    sums, counts = O.class_sums(np.abs(x), gt, C)
    return 2 * O.gamma(len(x) + 1) * sums / np.maximum(counts, 1)[:, None]


def cond_sym(a):
    ev = np.linalg.eigvalsh(a)
    return ev[-1] / ev[0] if ev[0] > 0 else np.inf


# ------------------------------------------------------------------------------------------------- means, scatter: exact
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("F", FS)
def test_means_and_scatter_equal_the_oracle_on_integers(cuda, F, N):
    rng = np.random.default_rng(100 * F + N)
    for C in CS:
        x = rng.integers(-64, 65, (N, F)).astype(np.float32)
        gt = labels(rng, N, C)
        mean, count = run_means(cuda, x, gt, C)
        want_mean, want_count = O.class_means(x, gt, C)
        assert np.array_equal(count, want_count) and np.array_equal(mean, want_mean), (C, "means")
        if C > 2 and N >= 5:
            assert count[C - 2] == 0 and not mean[C - 2].any()
        m_int = rng.integers(-64, 65, (C + 1, F)).astype(np.float64)
        for mode in (O.WITHIN, O.TOTAL):
            S = run_scatter(cuda, x, gt, m_int, C, mode).np()
            assert np.array_equal(S, O.scatter(x, gt, m_int, C, mode)), (C, mode)
            assert np.array_equal(S, S.T)
            assert np.array_equal(run_scatter(cuda, x, gt, m_int, C, mode).np(), S), "a second call"
            perm = rng.permutation(N)
            assert np.array_equal(run_scatter(cuda, x[perm], gt[perm], m_int, C, mode).np(), S), "permuted rows"
            if N >= 2:
                h = N // 2 if N < 100 else 37             # the second half's split differs from the whole call's
                acc = run_scatter(cuda, x[:h], gt[:h], m_int, C, mode)
                acc = run_scatter(cuda, x[h:], gt[h:], m_int, C, mode, into=acc).np()
                assert np.array_equal(acc, S), "two accumulate halves"


@pytest.mark.parametrize("N", (5, 257, 1031))
@pytest.mark.parametrize("F", FS)
def test_scatter_on_real_inputs_within_the_summation_bound(cuda, F, N):
    x, gt = blobs(7 * F + N, N, 3, F)
    mean, _ = run_means(cuda, x, gt, 3)
    assert (np.abs(mean - O.class_means(x, gt, 3)[0]) <= mean_bound(x, gt, 3)).all()
    for mode in (O.WITHIN, O.TOTAL):
        S = run_scatter(cuda, x, gt, mean, 3, mode).np()
        assert (np.abs(S - O.scatter(x, gt, mean, 3, mode)) <= O.scatter_bound(x, gt, mean, 3, mode)).all()
        assert np.array_equal(S, S.T)
        assert np.array_equal(run_scatter(cuda, x, gt, mean, 3, mode).np(), S)


# ------------------------------------------------------------------------------------------------------------------ factor
def spd_input(F, seed):
    rng = np.random.default_rng(seed)
    n = 3 * F + 10
    a = rng.standard_normal((n, F)) * np.linspace(0.5, 2.0, F)
    return a.T @ a, n


def check_factor(cuda, S, scale, shrinkage):
    F = len(S)
    L, W, logdet, info = run_factor(cuda, S, scale, shrinkage)
    assert info == 0
    assert not np.triu(L, 1).any() and not np.triu(W, 1).any()
    sg = O.sigma(S, scale, shrinkage)
    aL, aW, eye = np.abs(L), np.abs(W), np.eye(F)
    assert (np.abs(L @ L.T - sg) <= 2 * O.gamma(F + 8) * (aL @ aL.T)).all()
    assert (np.abs(W @ L - eye) <= 2 * O.gamma(F) * (aW @ aL)).all() or (np.abs(L @ W - eye) <= 2 * O.gamma(F) * (aL @ aW)).all()
    want, scale_ln = O.logdet_of_diagonal(np.diag(L))
    assert abs(logdet - want) <= O.gamma(2 * F) * scale_ln
    return L, W


@pytest.mark.parametrize("shrinkage", (0.0, 0.1, 1.0))
@pytest.mark.parametrize("F", FS)
def test_factor_backward_errors(cuda, F, shrinkage):
    S, n = spd_input(F, 50 + F)
    check_factor(cuda, S, 1.0 / n, shrinkage)


@pytest.mark.parametrize("F", FS)
def test_factor_refuses_singular_and_nan_input(cuda, F):
    """A zero matrix fails at pivot 1; a matrix of ones (rank 1: the second pivot is 1 - 1 * 1 = 0 exactly) at pivot 2; an identity with
    a block of ones behind column 70 at pivot 72, inside the second panel; a NaN in S at pivot 1 (the trace is NaN). L = W = 0, logdet NaN."""
    cases = [(np.zeros((F, F)), 0.0, 1), (np.zeros((F, F)), 1.0, 1)]
    if F >= 2:
        cases.append((np.ones((F, F)), 0.0, 2))
    if F >= 130:
        s = np.eye(F)
        s[70:, 70:] = 1.0
        cases.append((s, 0.0, 72))
    s = spd_input(F, 3)[0]
    s[F - 1, F - 1] = np.nan
    cases.append((s, 0.1, 1))
    for S, shrinkage, pivot in cases:
        L, W, logdet, info = run_factor(cuda, S, 1.0, shrinkage)
        assert info == pivot == O.factor(S, 1.0, shrinkage)[3]
        assert not L.any() and not W.any() and np.isnan(logdet)


def test_nan_feature_fails_the_fit(cuda):
    x, gt = blobs(5, 40, 3, 17)
    x[7, 3] = np.nan
    gt[7] = 0
    mean, _ = run_means(cuda, x, gt, 3)
    S = run_scatter(cuda, x, gt, mean, 3, O.WITHIN).np()
    assert np.isnan(S).any()
    L, W, logdet, info = run_factor(cuda, S, 1.0 / 40, 0.1)
    assert info > 0 and not L.any() and not W.any() and np.isnan(logdet)


# ------------------------------------------------------------------------------------------------------- whiten and sqdist
_FITS = {}


def device_fit(cuda, F, C=3, N=300, relative=True):
    """The whole fit through the C ABI on Gaussian blobs with shrinkage 0.1, once per shape, shared and left unchanged: the training
    arrays, the oracle's Fit and the device's (W, zm, W0, zm0)."""
    key = (F, C, N)
    if key not in _FITS:
        x, gt = blobs(1000 + F + C, N, C, F)
        gt_fit = np.where(gt >= C, -1, gt)                # the label C is not a class of this fit
        ref = O.Fit(x, gt_fit, 0.1, True)
        assert ref.C == C and ref.info == 0 and ref.info0 == 0
        assert cond_sym(ref.sigma) <= 1e4 and cond_sym(O.sigma(ref.S0, 1.0 / ref.counts[C], 0.1)) <= 1e4
        mean, count = run_means(cuda, x, gt_fit, C)
        n = int(count[C])
        dev = []
        for mode in (O.WITHIN, O.TOTAL):
            S = run_scatter(cuda, x, gt_fit, mean, C, mode).np()
            L, W = check_factor(cuda, S, 1.0 / n, 0.1)
            dev.append(W)
        zm = run_whiten(cuda, mean[:C], dev[0])
        zm0 = run_whiten(cuda, mean[C:], dev[1])
        for a in (x, mean, zm, zm0, dev[0], dev[1]):
            a.setflags(write=False)
        _FITS[key] = (x, ref, mean, dev[0], zm, dev[1], zm0)
    return _FITS[key]


def check_scores(got, ref, slack, what):
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= ulp32(ref) + slack).all(), (what, float((err / (ulp32(ref) + slack)).max()))


def check_against_fit(ref, q, dist, pred, unknown, relative):
    d, d0 = ref.parts(q)
    if not relative:
        want, slack = d, 0.0
        want_pred = O.transform(want, O.SIM_GAUSS, q.shape[1])
    else:
        want, slack = d - d0[:, None], 1e-8 * (d + d0[:, None])
        want_pred = O.transform(want, O.SIM_LOGISTIC, q.shape[1])
    check_scores(dist, want, slack, "distances")
    # the similarity's derivative is at most 1 / 2F (Gauss) or 1 / 8F (logistic): the slack of a cancelling distance scales with it
    check_scores(pred, want_pred, slack / (2.0 * q.shape[1]), "predict")
    check_scores(unknown, want.min(axis=1), slack.min(axis=1) if relative else 0.0, "unknown_score")
    if want.shape[1] > 1:
        two = np.sort(want, axis=1)[:, :2]
        assert ((two[:, 1] - two[:, 0]) > 1e-6 * np.abs(two).max(axis=1)).all(), "the oracle's own gap"
    assert np.array_equal(dist.argmin(axis=1), want.argmin(axis=1)), "arg-min class on every row"
    assert ((pred > 0) & (pred <= 1)).all()


def abi_scores(cuda, q, W, zm, W0, zm0, relative):
    z = run_whiten(cuda, q, W)
    minus = run_sqdist(cuda, run_whiten(cuda, q, W0), zm0, None, O.RAW, True)[:, 0].copy() if relative else None
    dist = run_sqdist(cuda, z, zm, minus, O.RAW)
    pred = run_sqdist(cuda, z, zm, minus, O.SIM_LOGISTIC if relative else O.SIM_GAUSS)
    return z, dist, pred


@pytest.mark.parametrize("M", NS)
@pytest.mark.parametrize("F", FS)
def test_scores_within_one_ulp_of_the_oracle(cuda, F, M):
    x, ref, mean, W, zm, W0, zm0 = device_fit(cuda, F)
    rng = np.random.default_rng(2000 + F + M)
    q = (x[np.arange(M) % len(x)] + 0.25 * rng.standard_normal((M, F))).astype(np.float32)      # rows of the blobs, jittered
    for relative in (False, True):
        z, dist, pred = abi_scores(cuda, q, W, zm, W0, zm0, relative)
        bound = 2 * O.gamma(F) * (np.abs(q).astype(np.float64) @ np.abs(W).T)
        assert (np.abs(z - O.whiten(q, W)) <= bound).all(), "whiten"
        check_against_fit(ref, q, dist, pred, dist.min(axis=1), relative)


@pytest.mark.parametrize("C", (1, 7))
def test_scores_other_class_counts(cuda, C):
    x, ref, mean, W, zm, W0, zm0 = device_fit(cuda, 65, C)
    q = (x[:70] + 0.25 * np.random.default_rng(31 + C).standard_normal((70, 65))).astype(np.float32)
    for relative in (False, True):
        z, dist, pred = abi_scores(cuda, q, W, zm, W0, zm0, relative)
        check_against_fit(ref, q, dist, pred, dist.min(axis=1), relative)


def test_sqdist_outputs_transforms_and_nan(cuda):
    """The fp64 output against the oracle on the same z (both sides within gamma_{F+1} of the exact sum of the same squares), the fp32
    output its single rounding, `minus`, the three transforms, and a NaN in z, zm or minus propagating through each of them."""
    rng = np.random.default_rng(9)
    M, C, F = 9, 5, 131
    z, zm, minus = rng.standard_normal((M, F)) * 3, rng.standard_normal((C, F)), rng.standard_normal(M) * 50
    z[2, 7] = np.nan
    zm[3, 130] = np.nan
    minus[5] = np.nan
    nan = np.zeros((M, C), dtype=bool)
    nan[2], nan[:, 3], nan[5] = True, True, True
    raw = O.sqdist(z, zm)
    for what in (O.RAW, O.SIM_GAUSS, O.SIM_LOGISTIC):
        for mi in (None, minus):
            want, v = O.sqdist(z, zm, mi, what), O.sqdist(z, zm, mi)
            assert np.isnan(want[2]).all() and np.isnan(want[:, 3]).all() and np.isnan(want[5]).all() == (mi is not None)
            got64, got32 = run_sqdist(cuda, z, zm, mi, what, True), run_sqdist(cuda, z, zm, mi, what)
            assert np.array_equal(np.isnan(got64), np.isnan(want)) and np.array_equal(np.isnan(got32), np.isnan(want))
            ok = ~np.isnan(want)
            slack = 2 * O.gamma(F + 1) * raw[ok] + 2 * O.U * np.abs(v[ok])             # the sums, then the one subtraction of minus
            if what != O.RAW:                             # |d similarity / d v| <= 1 / 2F; exp and the division round values <= 1
                slack = slack / (2.0 * F) + 4 * O.U
            assert (np.abs(got64 - want)[ok] <= slack).all()
            assert np.array_equal(got32[ok], got64.astype(np.float32)[ok])


def test_whiten_f64_equals_f32_on_fp32_values(cuda):
    x, ref, mean, W, zm, W0, zm0 = device_fit(cuda, 131)
    q = x[:70]
    assert np.array_equal(run_whiten(cuda, q, W), run_whiten(cuda, q.astype(np.float64), W))


# ------------------------------------------------------------------------------------------------------- workload's width
def test_workload_width(cuda):
    """F = 2048, N = 4096, C = 7, shrinkage 0.1: scatter, factor, whitening and scores at the size of the ResNet-50 features."""
    F, N, C = 2048, 4096, 7
    x, gt = blobs(77, N, C, F)
    gt = np.where(gt >= C, -1, gt)
    mean, count = run_means(cuda, x, gt, C)
    want_mean, want_count = O.class_means(x, gt, C)
    assert np.array_equal(count, want_count) and (np.abs(mean - want_mean) <= mean_bound(x, gt, C)).all()
    n = int(count[C])
    S = run_scatter(cuda, x, gt, mean, C, O.WITHIN).np()
    assert (np.abs(S - O.scatter(x, gt, mean, C, O.WITHIN)) <= O.scatter_bound(x, gt, mean, C, O.WITHIN)).all()
    assert np.array_equal(S, S.T)
    sg = O.sigma(S, 1.0 / n, 0.1)
    assert cond_sym(sg) <= 1e4
    L, W = check_factor(cuda, S, 1.0 / n, 0.1)
    zm = run_whiten(cuda, mean[:C], W)
    q = x[:67]
    z = run_whiten(cuda, q, W)
    assert (np.abs(z - O.whiten(q, W)) <= 2 * O.gamma(F) * (np.abs(q).astype(np.float64) @ np.abs(W).T)).all()
    dist, pred = run_sqdist(cuda, z, zm), run_sqdist(cuda, z, zm, None, O.SIM_GAUSS)
    Lr, Wr, _, info = O.factor(O.scatter(x, gt, want_mean, C, O.WITHIN), 1.0 / n, 0.1)
    assert info == 0
    want = O.sqdist(O.whiten(q, Wr), O.whiten(want_mean[:C], Wr))
    check_scores(dist, want, 0.0, "distances")
    check_scores(pred, O.transform(want, O.SIM_GAUSS, F), 0.0, "predict")
    two = np.sort(want, axis=1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) > 1e-6 * two[:, 1]).all()
    assert np.array_equal(dist.argmin(axis=1), want.argmin(axis=1))


# -------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("relative", (False, True))
def test_fit_and_scores_end_to_end(cuda, relative):
    from openset_imagenet import Mahalanobis
    N, F, C = 600, 96, 5
    x, gt = blobs(11, N, C, F)
    gt = np.where(gt >= C, -1, gt)
    ref = O.Fit(x, gt, 0.1, relative)
    assert ref.info == 0 and cond_sym(ref.sigma) <= 1e4
    maha = Mahalanobis(shrinkage=0.1, relative=relative).fit(x, torch.tensor(gt))
    assert np.array_equal(maha.counts.cpu().numpy(), ref.counts) and maha.whitened_means.shape == (C, F)
    assert maha.L.dtype == maha.W.dtype == maha.means.dtype == maha.logdet.dtype == torch.float64
    # d logdet = tr(Sigma^-1 dSigma) <= F cond |dSigma| / |Sigma|, the scatter's relative error at most 2 gamma_N on either side
    assert abs(float(maha.logdet) - ref.logdet) <= F * 1e4 * 4 * O.gamma(N)
    assert (maha.W0 is not None) == relative
    q = blobs(12, 203, C, F)[0]
    dist, pred, unknown = maha.distances(q), maha.predict(torch.tensor(q)), maha.unknown_score(q)
    assert dist.dtype == pred.dtype == unknown.dtype == torch.float32 and dist.is_cuda and unknown.shape == (203,)
    check_against_fit(ref, q, dist.cpu().numpy(), pred.cpu().numpy(), unknown.cpu().numpy(), relative)
    assert torch.equal(unknown, dist.min(dim=1).values)
    # chunked = unchunked, bit for bit; on the device as well as from the host
    assert torch.equal(maha.distances(q, chunk=64), dist) and torch.equal(maha.predict(torch.tensor(q).cuda(), chunk=5), pred)
    assert torch.equal(maha.unknown_score(q, chunk=100), unknown)
    # a chunked fit: the scatter accumulates row chunks; the same bounds hold
    chunked = Mahalanobis(shrinkage=0.1, relative=relative).fit(x, gt, chunk=250)
    check_against_fit(ref, q, chunked.distances(q).cpu().numpy(), chunked.predict(q).cpu().numpy(), chunked.unknown_score(q).cpu().numpy(),
                      relative)
    # the state dict round-trips: host tensors, moved on first use, the same bits out
    sd = maha.state_dict()
    assert all(v is None or not isinstance(v, torch.Tensor) or v.device.type == "cpu" for v in sd.values())
    again = Mahalanobis().load_state_dict(sd)
    assert again.relative is relative and again.W.device.type == "cpu"
    assert torch.equal(again.distances(q), dist) and again.W.is_cuda and torch.equal(again.predict(q), pred)


def test_fit_raises_on_a_covariance_that_is_not_positive_definite(cuda):
    """n - C < F with shrinkage 0: the scatter has rank n - C at most. Column 5 is dead (all zeros, as a ReLU channel can be), so the
    sixth pivot is an exact zero whatever the rounding of the others; a positive shrinkage repairs it."""
    from openset_imagenet import Mahalanobis
    x, gt = blobs(13, 60, 5, 96)
    gt = np.where(gt >= 5, -1, gt)
    x[:, 5] = 0.0
    with pytest.raises(ValueError, match=r"not positive definite \(pivot 6 of 96.*positive shrinkage"):
        Mahalanobis().fit(x, gt)
    with pytest.raises(ValueError, match="total covariance is not positive definite|within-class covariance is not positive definite"):
        Mahalanobis(relative=True).fit(x, gt)
    assert Mahalanobis(shrinkage=0.05).fit(x, gt).distances(x).shape == (60, 5)

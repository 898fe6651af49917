"""numpy fp64 restatement of the Mahalanobis / Relative Mahalanobis scores as include/osi.h (ABI 25) defines them: class means, the
centred scatter, Sigma and its Cholesky factor and inverse, whitening, squared distances and their three transforms, and the whole of
Mahalanobis.fit / distances / predict / unknown_score on top. A helper of tests/test_mahalanobis_cpu.py and
tests/test_mahalanobis_gpu.py, not collected as a test. With scipy present the inverse is a triangular solve, otherwise a solve against
the identity."""
import numpy as np

try:
    from scipy.linalg import solve_triangular
except ImportError:                                       # pragma: no cover
    solve_triangular = None

WITHIN, TOTAL = 0, 1
RAW, SIM_GAUSS, SIM_LOGISTIC = 0, 1, 2
MAX_F = 32768
U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


def counted(gt, C):
    gt = np.asarray(gt, dtype=np.int64)
    return (gt >= 0) & (gt < C)


def class_sums(x, gt, C):
    """sums [C + 1, F] fp64 and counts [C + 1] int64; row C over all counted rows."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    gt = np.asarray(gt, dtype=np.int64)
    sums = np.zeros((C + 1, x.shape[1]))
    counts = np.zeros(C + 1, dtype=np.int64)
    for c in range(C):
        sums[c] = x[gt == c].sum(axis=0)
        counts[c] = int((gt == c).sum())
    keep = counted(gt, C)
    sums[C] = x[keep].sum(axis=0)
    counts[C] = int(keep.sum())
    return sums, counts


def class_means(x, gt, C):
    sums, counts = class_sums(x, gt, C)
    mean = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], 0.0)
    return mean, counts


def centred(x, gt, mean, C, mode):
    """a [n, F]: the counted rows, (double)x - m in one rounded subtraction."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    gt = np.asarray(gt, dtype=np.int64)
    keep = counted(gt, C)
    m = mean[gt[keep]] if mode == WITHIN else mean[C][None, :]
    return x[keep] - m


def scatter(x, gt, mean, C, mode):
    a = centred(x, gt, mean, C, mode)
    return a.T @ a


def scatter_bound(x, gt, mean, C, mode):
    """2 gamma_n sum_k |a_ki| |a_kj|: both sides are within gamma_n of the exact sum of identical products."""
    a = np.abs(centred(x, gt, mean, C, mode))
    return 2.0 * gamma(max(len(a), 1)) * (a.T @ a)


def sigma(S, scale, shrinkage):
    F = S.shape[0]
    return (1.0 - shrinkage) * scale * S + shrinkage * (scale * np.trace(S) / F) * np.eye(F)


def factor(S, scale, shrinkage):
    """(L, W, logdet, info): info = 0 and the factor, or info > 0 (the first failed pivot, found by an unblocked walk), zeros and NaN."""
    F = S.shape[0]
    sg = sigma(S, scale, shrinkage)
    try:
        if not np.isfinite(sg).all():
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(sg)
    except np.linalg.LinAlgError:
        return np.zeros((F, F)), np.zeros((F, F)), np.nan, first_bad_pivot(sg)
    W = solve_triangular(L, np.eye(F), lower=True) if solve_triangular is not None else np.linalg.solve(L, np.eye(F))
    return L, np.tril(W), 2.0 * np.log(np.diag(L)).sum(), 0


def first_bad_pivot(sg):
    a = np.array(sg, dtype=np.float64)
    F = len(a)
    with np.errstate(all="ignore"):
        for j in range(F):
            p = a[j, j]
            if not (p > 0) or p == np.inf:
                return j + 1
            d = np.sqrt(p)
            a[j + 1:, j] /= d
            a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j + 1:, j])
    return 0


def logdet_of_diagonal(diag):
    """2 sum ln d in extended precision: the reference of the logdet bound, free of its own rounding at the bound's scale."""
    d = np.asarray(diag, dtype=np.longdouble)
    return float(2 * np.log(d).sum()), float(np.abs(np.log(d)).sum())


def whiten(x, W):
    return np.asarray(x, dtype=np.float64) @ np.tril(W).T


def transform(v, what, F):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if what == RAW:
            return v
        if what == SIM_GAUSS:
            return np.where(np.isnan(v), v, np.exp(-np.maximum(v, 0.0) / (2.0 * F)))
        if what == SIM_LOGISTIC:
            return 1.0 / (1.0 + np.exp(v / (2.0 * F)))
    raise ValueError(what)


def sqdist(z, zm, minus=None, what=RAW):
    """fp64 [M, C]: sum_j (z_ij - zm_cj)^2 in the difference form, minus[i] subtracted, then the transform."""
    z, zm = np.asarray(z, dtype=np.float64), np.asarray(zm, dtype=np.float64)
    v = np.empty((len(z), len(zm)))
    for c in range(len(zm)):
        d = z - zm[c]
        v[:, c] = (d * d).sum(axis=1)
    if minus is not None:
        v = v - np.asarray(minus, dtype=np.float64)[:, None]
    return transform(v, what, z.shape[1])


class Fit:
    """Mahalanobis.fit restated: means, counts, L, W, logdet, whitened means and, when relative, the background set."""

    def __init__(self, x, gt, shrinkage=0.0, relative=False):
        gt = np.asarray(gt, dtype=np.int64)
        self.C = int(gt.max()) + 1
        self.relative = relative
        self.means, self.counts = class_means(x, gt, self.C)
        n = int(self.counts[self.C])
        self.S = scatter(x, gt, self.means, self.C, WITHIN)
        self.sigma = sigma(self.S, 1.0 / n, shrinkage)
        self.L, self.W, self.logdet, self.info = factor(self.S, 1.0 / n, shrinkage)
        self.whitened_means = whiten(self.means[:self.C], self.W)
        if relative:
            self.S0 = scatter(x, gt, self.means, self.C, TOTAL)
            self.L0, self.W0, self.logdet0, self.info0 = factor(self.S0, 1.0 / n, shrinkage)
            self.whitened_mean0 = whiten(self.means[self.C:], self.W0)

    def parts(self, x):
        """(d2 to the class means [M, C], d2 under the background Gaussian [M] or None), fp64."""
        x = np.asarray(x, dtype=np.float32).astype(np.float64)
        d = sqdist(whiten(x, self.W), self.whitened_means)
        d0 = sqdist(whiten(x, self.W0), self.whitened_mean0)[:, 0] if self.relative else None
        return d, d0

    def distances(self, x):
        d, d0 = self.parts(x)
        return d if d0 is None else d - d0[:, None]

    def predict(self, x):
        return transform(self.distances(x), SIM_LOGISTIC if self.relative else SIM_GAUSS, self.W.shape[0])

    def unknown_score(self, x):
        return self.distances(x).min(axis=1)

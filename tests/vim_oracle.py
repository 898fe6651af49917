"""numpy fp64 restatement of ViM and of the symmetric eigensolver under it (include/osi.h ABI 26, openset_imagenet/vim.py): what the
GPU tests compare against. The eigen-decomposition of the oracle is np.linalg.eigh; `jacobi` restates the device's parallel cyclic
Jacobi (the same ordering, angles, threshold and update order) and is used on the CPU only, to show that the inputs of the GPU tests
converge. Also here: the inputs themselves, so that the CPU and the GPU tests see the same matrices."""
import numpy as np

U = 2.0 ** -53
NORM, UNKNOWN, PROBS = 0, 1, 2
MAX_F = 4096
MAX_SWEEPS = 30


def gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------------------ eigensolver
def partners(F, r):
    """Round r of the round-robin ordering over n = F rounded up to even players: partner[j] for every column j < F (the bye of an
    odd F is its own partner), and the pairs p < q (both < F) as two arrays."""
    n = F + (F & 1)
    n1 = n - 1
    j = np.arange(F)
    k = (2 * r - j) % n1
    k = np.where(j == n1, r, np.where(j == r, n1, k))
    k = np.where(k >= F, j, k)
    p = j[j < k]
    return k, p, k[p]


def rounds_of(F):
    return F + (F & 1) - 1


def eigh_error(F, sweeps):
    """(10 r u + F 2^-52) with r = 2 s (F - 1) rotation stages: the bound on |S V - V L|_F / |S|_F. A rotation applied to a 2-vector has
    error <= 10 u of its norm (6 u from two products and a sum with computed c and s, 4 u from forming them); the second term is the
    off-diagonal mass the threshold leaves."""
    return 10.0 * (2 * sweeps * (F - 1)) * U + F * 2.0 ** -52


def orth_error(F, sweeps):
    return 20.0 * sweeps * (F - 1) * U * np.sqrt(F)


def jacobi(S, max_sweeps=MAX_SWEEPS, vectors=True):
    """(values descending, vectors as rows with the sign rule, sweeps run); sweeps = None when max_sweeps did not converge. A whole
    round at once: rows, then columns, then the exact zeros, every angle from the matrix as the previous round left it.
    vectors=False leaves the vectors at the identity (a third of the work, for a convergence count alone)."""
    A = np.array(S, dtype=np.float64)
    F = len(A)
    Vt = np.eye(F)
    norm = np.sqrt((A * A).sum())
    if not np.isfinite(norm):
        return np.full(F, np.nan), np.zeros((F, F)), 0
    tau = norm * 2.0 ** -52
    done = None
    for sweep in range(1, max_sweeps + 1):
        rotations = 0
        for r in range(rounds_of(F)):
            k, p, q = partners(F, r)
            apq = A[p, q]
            rot = np.abs(apq) > tau
            rotations += int(rot.sum())
            if not rot.any():
                continue
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            t = np.where(rot, t, 0.0)
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            cc, ss = np.ones(F), np.zeros(F)
            cc[p], cc[q], ss[p], ss[q] = c, c, -s, s
            A = cc[:, None] * A + ss[:, None] * A[k]
            A = cc[None, :] * A + ss[None, :] * A[:, k]
            A[p[rot], q[rot]] = 0.0
            A[q[rot], p[rot]] = 0.0
            if vectors:
                Vt = cc[:, None] * Vt + ss[:, None] * Vt[k]
        if rotations == 0:
            done = sweep
            break
    d = np.diag(A)
    order = np.argsort(-d, kind="stable")
    return d[order], signed(Vt[order]), done


def signed(rows):
    """Every row with its entry of largest magnitude (the first of equals) positive."""
    at = np.abs(rows).argmax(axis=1)
    flip = rows[np.arange(len(rows)), at] < 0
    return np.where(flip[:, None], -rows, rows)


def eigh(S):
    """np.linalg.eigh, descending, eigenvectors as rows, the sign rule."""
    w, v = np.linalg.eigh(np.asarray(S, dtype=np.float64))
    return w[::-1].copy(), signed(v.T[::-1])


def planted_rows(F, n, sigma, seed, offset=0.0):
    """n rows with standard deviations `sigma` along the columns of a random orthogonal basis, plus `offset` on every column."""
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((F, F)))[0]
    return (rng.standard_normal((n, F)) * np.asarray(sigma)) @ q.T + offset


PLANTED_F = (1, 2, 3, 15, 16, 17, 63, 64, 65, 130, 131, 515)
SPECIAL_F = 33
SPECIALS = ("zeros", "identity", "ones", "diag_ascending", "repeated", "rank_deficient")


def eigh_input(name, F):
    """The eigensolver inputs of the tests: second moments of planted-spectrum rows, and the special matrices."""
    if name == "planted":
        x = planted_rows(F, 3 * F + 10, np.geomspace(2.0, 0.05, F), 40 + F)
        return x.T @ x
    if name == "zeros":
        return np.zeros((F, F))
    if name == "identity":
        return np.eye(F)
    if name == "ones":
        return np.ones((F, F))
    if name == "diag_ascending":
        return np.diag(np.arange(1.0, F + 1.0))
    if name == "repeated":
        q = np.linalg.qr(np.random.default_rng(7).standard_normal((F, F)))[0]
        a = q @ np.diag(np.repeat([5.0, 2.0, 0.5], [3, F // 2, F - 3 - F // 2])) @ q.T
        return (a + a.T) / 2
    if name == "rank_deficient":                          # n < F rows and one dead column
        x = planted_rows(F, F // 2, np.linspace(2.0, 0.5, F), 9)
        x[:, 5] = 0.0
        return x.T @ x
    raise KeyError(name)


EIGH_CASES = tuple(("planted", F) for F in PLANTED_F) + tuple((name, SPECIAL_F) for name in SPECIALS)


# -------------------------------------------------------------------------------------------------------------------- ViM
def default_dim(F):
    return 1000 if F >= 2048 else 512 if F >= 768 else F // 2


def logit_origin(weight, bias):
    return -np.linalg.pinv(np.asarray(weight, dtype=np.float64)) @ np.asarray(bias, dtype=np.float64)


def second_moment(x, origin, gt=None):
    a = x.astype(np.float64) - origin
    if gt is not None:
        a = a[np.asarray(gt) >= 0]
    return a.T @ a


def project(x, origin, R):
    return (x.astype(np.float64) - origin) @ R.T


def logsumexp(lg):
    lg = lg.astype(np.float64)
    mx = lg.max(axis=1)
    shift = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore"):
        return shift + np.log(np.exp(lg - shift[:, None]).sum(axis=1))


def scores(z, logits, alpha, mode):
    """The three outputs of osi_vim_scores in fp64."""
    n = np.sqrt((z * z).sum(axis=1))
    if mode == NORM:
        return n
    v = alpha * n
    if mode == UNKNOWN:
        return v - logsumexp(logits)
    full = np.concatenate([logits.astype(np.float64), v[:, None]], axis=1)
    mx = np.fmax.reduce(full, axis=1)
    e = np.exp(full - np.where(np.isfinite(mx), mx, 0.0)[:, None])
    return e / e.sum(axis=1, keepdims=True)


E2E_F, E2E_DIM, E2E_C = 96, 48, 5


def e2e_data(seed=21, n=600):
    """The end-to-end case: rows with a planted gap at E2E_DIM (sigma 3 -> 2 | 0.5 -> 0.05 along a random orthogonal basis, offset 0.5 on
    the principal coordinates), a last layer with a bias (so the origin is not zero) whose rows lie in the principal subspace, its logits,
    labels with a few negatives. The mean and the origin inside the principal subspace keep the second moment ABOUT THE ORIGIN from
    growing a large eigenvalue past the cut. Returns x, logits (fp32), gt, weight, bias. The basis is the same for every seed."""
    sigma = np.concatenate([np.linspace(3.0, 2.0, E2E_DIM), np.linspace(0.5, 0.05, E2E_F - E2E_DIM)])
    basis = np.linalg.qr(np.random.default_rng(20).standard_normal((E2E_F, E2E_F)))[0]
    rng = np.random.default_rng(seed + 1)
    shift = np.concatenate([np.full(E2E_DIM, 0.5), np.zeros(E2E_F - E2E_DIM)])
    x = ((rng.standard_normal((n, E2E_F)) * sigma + shift) @ basis.T).astype(np.float32)
    weight, bias = 0.2 * rng.standard_normal((E2E_C, E2E_DIM)) @ basis[:, :E2E_DIM].T, rng.standard_normal(E2E_C)
    logits = (x.astype(np.float64) @ weight.T + bias).astype(np.float32)
    gt = rng.integers(0, E2E_C, n)
    gt[::17] = -1
    gt[5] = -2
    return x, logits, gt.astype(np.int64), weight, bias


class Fit:
    def __init__(self, x, logits, gt=None, origin=None, dim=None):
        F = x.shape[1]
        self.origin = np.zeros(F) if origin is None else np.asarray(origin, dtype=np.float64)
        self.dim = default_dim(F) if dim is None else dim
        keep = np.ones(len(x), dtype=bool) if gt is None else np.asarray(gt) >= 0
        self.count = int(keep.sum())
        self.S = second_moment(x[keep], self.origin)
        self.eigenvalues, self.components = eigh(self.S)
        self.R = self.components[self.dim:]
        n = self.residual_norm(x[keep])
        self.alpha = float(logits[keep].astype(np.float64).max(axis=1).sum() / n.sum())

    def residual_norm(self, x):
        return scores(project(x, self.origin, self.R), None, 0.0, NORM)

    def unknown_score(self, x, logits):
        return scores(project(x, self.origin, self.R), logits, self.alpha, UNKNOWN)

    def probabilities(self, x, logits):
        return scores(project(x, self.origin, self.R), logits, self.alpha, PROBS)

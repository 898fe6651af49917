"""fp64 numpy restatement of the Extreme Value Machine as include/osi.h (ABI 22) defines it: all-pairs distances, the per-row tail and
its Weibull fit (libMR's FitLow), the inclusion probability, the greedy set cover and the class scores. A helper of
tests/test_evm_cpu.py and tests/test_evm_gpu.py, not collected as a test. The Weibull solver is openmax_oracle's bisection to bracket
exhaustion."""
import numpy as np

from openmax_oracle import ordered_sum, weibull_fit

EUCLIDEAN, COSINE = 0, 1


# ------------------------------------------------------------------------------------------------------------- distances
def sq_norms(x):
    """Squared row norms, fp64 sums in index order."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return ordered_sum(x * x, axis=1)


def dots(a, b):
    """a_i . b_j in fp64 (exact for small integers, where the device's fp32 chain is exact too)."""
    a, b = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return a @ b.T


def distances(a, b, metric, dot=None):
    """[R, N] fp32. `dot` (fp32 [R, N]) replaces the fp64 dot products when given."""
    naa, nbb = sq_norms(a)[:, None], sq_norms(b)[None, :]
    dot = dots(a, b) if dot is None else np.asarray(dot, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if metric == COSINE:
            d = 1.0 - dot / np.sqrt(naa * nbb)
        else:
            t = (naa + nbb) - 2.0 * dot
            d = np.sqrt(np.where(t < 0, 0.0, t))                            # a NaN passes the clamp
        return d.astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- fit rows
def scaled(dist, multiplier):
    """y = -(multiplier * d), the product rounded to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        return -(np.float32(multiplier) * np.asarray(dist, dtype=np.float32))


def fit_low(y, T):
    """The tail fit of osi_openmax_fit_tails on the finite candidates y (fp32): (shape, scale, shift, fitted, tail_count)."""
    tail = np.sort((np.asarray(y, dtype=np.float32) + np.float32(0)).astype(np.float64))[-T:]      # -0 + 0 = +0
    if len(tail) < 2 or tail[0] == tail[-1] or tail[-1] - tail[0] + 1.0 == 1.0:
        return 0.0, 0.0, 0.0, 0, len(tail)
    k, lam = weibull_fit(tail - tail[0] + 1.0)
    return k, lam, tail[0], 1, len(tail)


def fit_rows(dist, N, gt, cls, T, multiplier):
    """dict(shape, scale, shift fp64 [R]; fitted uint8 [R]; tail_count int64 [R]; flags2 int64 [2]) from dist [R, ld >= N]."""
    dist, gt = np.asarray(dist, dtype=np.float32)[:, :N], np.asarray(gt).astype(np.int64)[:N]
    R = len(dist)
    out = dict(shape=np.zeros(R), scale=np.zeros(R), shift=np.zeros(R), fitted=np.zeros(R, dtype=np.uint8),
               tail_count=np.zeros(R, dtype=np.int64), flags2=np.zeros(2, dtype=np.int64))
    for r in range(R):
        y = scaled(dist[r][gt != cls], multiplier)
        finite = np.isfinite(y)
        out["flags2"][0] += int((~finite).sum())
        out["shape"][r], out["scale"][r], out["shift"][r], out["fitted"][r], out["tail_count"][r] = fit_low(y[finite], T)
        out["flags2"][1] += 1 - int(out["fitted"][r])
    return out


# ------------------------------------------------------------------------------------------------- inclusion probability
def psi(d, multiplier, shape, scale, shift, fitted):
    """Psi of distances d against parameters that broadcast with d; fp32. 0 for z <= 0 or unfitted, NaN for a NaN d."""
    d = np.asarray(d, dtype=np.float32)
    z = scaled(d, multiplier).astype(np.float64) - shift + 1.0
    fitted = np.broadcast_to(np.asarray(fitted).astype(bool), z.shape)
    live = fitted & (z > 0)
    with np.errstate(all="ignore"):
        k, lam = np.where(fitted, shape, 1.0), np.where(fitted, scale, 1.0)
        p = 1.0 - np.exp(-(np.where(live, z, 1.0) / lam) ** k)
    p = np.where(live, p, 0.0)
    return np.where(np.isnan(d), np.nan, p).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- set cover
def cover_matrix(dpp, shape, scale, shift, fitted, multiplier, threshold):
    """bool [R, R]: row i covers row j."""
    fitted = np.asarray(fitted).astype(bool)
    p = psi(dpp, multiplier, shape[:, None], scale[:, None], shift[:, None], fitted[:, None])
    with np.errstate(invalid="ignore"):
        cov = (p >= np.float32(threshold)) | np.eye(len(fitted), dtype=bool)
    return cov & fitted[:, None] & fitted[None, :]


def greedy_cover(cov, fitted):
    """(order int64 [R] padded with -1, n_ev): the counts are kept up to date as the device keeps them."""
    cov, fitted = np.asarray(cov, dtype=bool), np.asarray(fitted).astype(bool)
    R = len(fitted)
    U = fitted.copy()
    cnt = (cov & U[None, :]).sum(axis=1)
    order = np.full(R, -1, dtype=np.int64)
    n = 0
    while U.any():
        p = int(np.argmax(cnt))                                             # the first maximum: the lowest index on ties
        assert cnt[p] > 0
        newly = cov[p] & U
        U &= ~newly
        cnt = cnt - (cov & newly[None, :]).sum(axis=1)
        order[n] = p
        n += 1
    return order, n


def set_cover(dpp, shape, scale, shift, fitted, multiplier, threshold):
    return greedy_cover(cover_matrix(dpp, shape, scale, shift, fitted, multiplier, threshold), fitted)


# ----------------------------------------------------------------------------------------------------------------- probs
def probs(dist, V, shape, scale, shift, ev_start, multiplier):
    """[M, C] fp32: the maximum of Psi over a class's extreme vectors, 0 without any, NaN if any term is NaN."""
    dist = np.asarray(dist, dtype=np.float32)[:, :V]
    C = len(ev_start) - 1
    p = psi(dist, multiplier, shape[None, :], scale[None, :], shift[None, :], (np.asarray(scale) != 0)[None, :])
    out = np.zeros((len(dist), C), dtype=np.float32)
    for c in range(C):
        if ev_start[c + 1] > ev_start[c]:
            out[:, c] = np.maximum(np.max(p[:, ev_start[c]:ev_start[c + 1]], axis=1), np.float32(0))     # np.max keeps a NaN
    return out


# ---------------------------------------------------------------------------------------------------------- whole method
def fit(features, gt, T, multiplier, metric, threshold=None, use_negatives=True, dist_fn=None):
    """The whole of EVM.fit: dict(ev_features, ev_shape, ev_scale, ev_shift, ev_start, flags, ev_rows = the row index of every extreme
    vector in `features`). dist_fn(a, b) replaces the oracle's distances when given (the device's, for real-valued features)."""
    features, gt = np.asarray(features, dtype=np.float32), np.asarray(gt).astype(np.int64)
    dist_fn = dist_fn or (lambda a, b: distances(a, b, metric))
    C = int(gt.max()) + 1
    index = np.arange(len(gt))
    if not use_negatives:
        keep = (gt >= 0) & (gt < C)
        features, gt, index = features[keep], gt[keep], index[keep]
    ev = dict(rows=[], shape=[], scale=[], shift=[])
    start, flags = [0], np.zeros(2, dtype=np.int64)
    for c in range(C):
        idx = np.flatnonzero(gt == c)
        if len(idx):
            x = features[idx]
            m = fit_rows(dist_fn(x, features), len(gt), gt, c, T, multiplier)
            flags += m["flags2"]
            if threshold is None:
                sel = np.flatnonzero(m["fitted"])
            else:
                order, n = set_cover(dist_fn(x, x), m["shape"], m["scale"], m["shift"], m["fitted"], multiplier, threshold)
                sel = order[:n]
            ev["rows"].append(idx[sel])
            for k in ("shape", "scale", "shift"):
                ev[k].append(m[k][sel])
        start.append(start[-1] + (len(ev["rows"][-1]) if len(idx) else 0))
    rows = np.concatenate(ev["rows"]) if ev["rows"] else np.zeros(0, dtype=np.int64)
    cat = lambda k: np.concatenate(ev[k]) if ev[k] else np.zeros(0)
    return dict(ev_features=features[rows], ev_rows=index[rows], ev_shape=cat("shape"), ev_scale=cat("scale"), ev_shift=cat("shift"),
                ev_start=np.asarray(start, dtype=np.int64), flags=flags)


def predict(model, features, multiplier, metric, dist_fn=None):
    dist_fn = dist_fn or (lambda a, b: distances(a, b, metric))
    V = len(model["ev_shape"])
    if V == 0:
        return np.zeros((len(features), len(model["ev_start"]) - 1), dtype=np.float32)
    return probs(dist_fn(features, model["ev_features"]), V, model["ev_shape"], model["ev_scale"], model["ev_shift"], model["ev_start"],
                 multiplier)


# ------------------------------------------------------------------------------------------- inputs shared by the tests
def make_features(R, F, seed, integer):
    """fp32 [R, F]: integers with |value| <= 4 (dot products and norms exact in fp32 up to F = 2^19), or real values."""
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-4, 5, (R, F)).astype(np.float32)
    return (rng.standard_normal((R, F)) * (0.5 + rng.random((R, 1)))).astype(np.float32)


def make_labels(N, C, seed):
    """int64 [N]: classes 0 .. C-1 (every one present when N >= 2 C) with -1, -2, C and C + 2 among them."""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, C, N)
    odd = rng.random(N)
    gt[odd < 0.06] = -1
    gt[(odd >= 0.06) & (odd < 0.10)] = -2
    gt[(odd >= 0.10) & (odd < 0.13)] = C
    gt[(odd >= 0.13) & (odd < 0.15)] = C + 2
    if N >= 2 * C:
        gt[:C] = np.arange(C)
    return gt.astype(np.int64)


def make_case(N, C, F, seed, integer):
    """(features fp32 [N, F], gt int64 [N]) for EVM.fit: labels 0 .. C-1 and -1, -2 (labels above the largest known one would be
    classes of their own). integer: |value| <= 4; otherwise one centre per label with unit noise."""
    rng = np.random.default_rng(seed)
    gt = make_labels(N, C, seed)
    gt[gt >= C] = -1
    if integer:
        features = rng.integers(-4, 5, (N, F)).astype(np.float32)
    else:
        centres = 2 * rng.standard_normal((C + 2, F))
        features = (centres[gt + 2] + rng.standard_normal((N, F))).astype(np.float32)
    return features, gt

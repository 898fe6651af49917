"""fp64 numpy restatement of OpenMax as include/osi.h (ABI 21) defines it: correct rows and class means, the two distances, the
tail and its Weibull fit, the w-score and the recalibration. A helper of tests/test_openmax_cpu.py and tests/test_openmax_gpu.py,
not collected as a test. The likelihood equation is solved by bisection until the bracket is exhausted, so the root does not depend
on a stopping rule."""
import numpy as np

EUCLIDEAN, COSINE = 0, 1


def ordered_sum(a, axis=-1):
    """Sum in index order (np.sum adds pairwise): the last entry of the running sum."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def correct_rows(logits, gt):
    """correct[i]: gt[i] in [0, C), no NaN in the row, and the first maximum is column gt[i]."""
    logits, gt = np.asarray(logits), np.asarray(gt).astype(np.int64)
    C = logits.shape[1]
    nan = np.isnan(logits).any(axis=1)
    arg = np.argmax(np.where(nan[:, None], 0, logits), axis=1)          # np.argmax: the first maximum
    return (gt >= 0) & (gt < C) & ~nan & (arg == gt)


def class_means(features, logits, gt):
    """(mav fp32 [C, F], count int64 [C], correct bool [N]); a class without a correct row gets zeros."""
    features, gt = np.asarray(features, dtype=np.float32), np.asarray(gt).astype(np.int64)
    C, F = np.asarray(logits).shape[1], features.shape[1]
    correct = correct_rows(logits, gt)
    mav, count = np.zeros((C, F), dtype=np.float32), np.zeros(C, dtype=np.int64)
    for c in range(C):
        rows = features[correct & (gt == c)].astype(np.float64)         # ascending row order
        count[c] = len(rows)
        if len(rows):
            mav[c] = (ordered_sum(rows, axis=0) / np.float64(len(rows))).astype(np.float32)
    return mav, count, correct


def distance(f, m, metric):
    """d(f, m) over the last axis (broadcasting), fp64 sums in index order, rounded once to fp32."""
    f, m = np.asarray(f, dtype=np.float32).astype(np.float64), np.asarray(m, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == EUCLIDEAN:
            d = np.sqrt(ordered_sum((f - m) ** 2))
        else:
            f, m = np.broadcast_arrays(f, m)
            d = 1.0 - ordered_sum(f * m) / np.sqrt(ordered_sum(f * f) * ordered_sum(m * m))
    return d.astype(np.float32)


def distances(features, mav, cls, metric):
    """cls None: [N, C]; otherwise [N], NaN where cls[i] is outside [0, C)."""
    features, mav = np.asarray(features, dtype=np.float32), np.asarray(mav, dtype=np.float32)
    if cls is None:
        return distance(features[:, None, :], mav[None, :, :], metric)
    cls = np.asarray(cls).astype(np.int64)
    ok = (cls >= 0) & (cls < len(mav))
    out = np.full(len(features), np.nan, dtype=np.float32)
    out[ok] = distance(features[ok], mav[cls[ok]], metric)
    return out


def weibull_g(k, lnx):
    """g(k) = sum x^k ln x / sum x^k - 1/k - mean(ln x), x^k as exp(k ln x - max)."""
    e = np.exp(k * lnx - np.max(k * lnx))
    return np.sum(e * lnx) / np.sum(e) - 1.0 / k - np.mean(lnx)


def weibull_fit(x):
    """(k, lambda) of the two-parameter Weibull maximum-likelihood fit to x >= 1 (not all equal): bisection on the increasing g to
    bracket exhaustion."""
    lnx = np.log(np.asarray(x, dtype=np.float64))
    lo = hi = 1.0
    if weibull_g(1.0, lnx) < 0:
        while weibull_g(hi, lnx) < 0:
            lo, hi = hi, hi * 2.0
    else:
        while weibull_g(lo, lnx) >= 0:
            hi, lo = lo, lo * 0.5
    while True:
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if weibull_g(mid, lnx) < 0:
            lo = mid
        else:
            hi = mid
    k = hi
    e = np.exp(k * lnx - np.max(k * lnx))
    lam = np.exp(np.max(lnx)) * np.mean(e) ** (1.0 / k)
    return k, lam


def fit_tails(dist, gt, correct, C, T):
    """dict(shape, scale, shift fp64 [C]; fitted uint8 [C]; tail_count int64 [C]; flags2 int64 [2])."""
    dist, gt, correct = np.asarray(dist, dtype=np.float32), np.asarray(gt).astype(np.int64), np.asarray(correct).astype(bool)
    shape, scale, shift = np.zeros(C), np.zeros(C), np.zeros(C)
    fitted, tail_count, flags2 = np.zeros(C, dtype=np.uint8), np.zeros(C, dtype=np.int64), np.zeros(2, dtype=np.int64)
    for c in range(C):
        d = dist[correct & (gt == c)]
        finite = np.isfinite(d)
        flags2[0] += int((~finite).sum())
        tail = np.sort(d[finite].astype(np.float64))[-T:]
        tail_count[c] = len(tail)
        if len(tail) < 2 or tail[0] == tail[-1] or tail[-1] - tail[0] + 1.0 == 1.0:     # equal ends, also after the translation
            flags2[1] += 1
            continue
        x = tail - tail[0] + 1.0
        shape[c], scale[c] = weibull_fit(x)
        shift[c], fitted[c] = tail[0], 1
    return dict(shape=shape, scale=scale, shift=shift, fitted=fitted, tail_count=tail_count, flags2=flags2)


def wscores(dist, shape, scale, shift, fitted):
    """[N, C] fp32; 0 for z <= 0 or an unfitted class, NaN for a NaN distance."""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    fitted = np.asarray(fitted).astype(bool)
    z = d - shift[None, :] + 1.0
    live = fitted[None, :] & (z > 0)
    with np.errstate(all="ignore"):
        k, lam = np.where(fitted, shape, 1.0), np.where(fitted, scale, 1.0)
        w = 1.0 - np.exp(-(np.where(live, z, 1.0) / lam[None, :]) ** k[None, :])
    w = np.where(live, w, 0.0)
    return np.where(np.isnan(d), np.nan, w).astype(np.float32)


def recalibrate(logits, w, alpha):
    """[N, C + 1] fp32, the unknown column last; a row with a NaN logit is NaN throughout."""
    v, w = np.asarray(logits, dtype=np.float32).astype(np.float64), np.asarray(w, dtype=np.float32).astype(np.float64)
    n, C = v.shape
    a = min(int(alpha), C)
    out = np.empty((n, C + 1), dtype=np.float32)
    for i in range(n):
        if np.isnan(v[i]).any():
            out[i] = np.nan
            continue
        order = np.argsort(-v[i], kind="stable")                        # descending, the lower index first on ties
        omega = np.ones(C)
        for r in range(a):
            omega[order[r]] = 1.0 - w[i, order[r]] * (a - r) / a
        with np.errstate(all="ignore"):
            hat = np.concatenate([v[i] * omega, [np.sum(v[i] * (1.0 - omega))]])
            e = np.exp(hat - np.max(hat))
            out[i] = (e / np.sum(e)).astype(np.float32)
    return out


def fit(features, logits, gt, T, metric):
    """The whole of OpenMax.fit: dict with mav, count, correct and the entries of fit_tails."""
    mav, count, correct = class_means(features, logits, gt)
    dist = distances(features, mav, gt, metric)
    out = fit_tails(dist, gt, correct, len(mav), T)
    out.update(mav=mav, count=count, correct=correct, dist=dist)
    return out


def predict(model, logits, features, alpha, metric, dist=None):
    """The whole of OpenMax.predict on a dict of fit(); `dist` replaces the [M, C] distances when given."""
    if dist is None:
        dist = distances(features, model["mav"], None, metric)
    w = wscores(dist, model["shape"], model["scale"], model["shift"], model["fitted"])
    return recalibrate(logits, w, alpha)


# ------------------------------------------------------------------------------------------- inputs shared by the tests
SHAPES = [(600, 7, 33), (97, 3, 1), (64, 1, 5), (300, 5, 130)]


def make_case(N, C, F, seed, integer):
    """(features fp32 [N, F], logits fp32 [N, C], gt int64 [N]): about three rows in four correct, labels -1, -2, C and C + 3
    among them, tied maxima (integer-valued logits), one row with a NaN logit. integer: features are integers with |value| <= 3
    (their fp64 sums are exact); otherwise real values clustered around one centre per class."""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, C, N)
    odd = rng.random(N)
    gt[odd < 0.06] = -1
    gt[(odd >= 0.06) & (odd < 0.10)] = -2
    gt[(odd >= 0.10) & (odd < 0.13)] = C
    gt[(odd >= 0.13) & (odd < 0.15)] = C + 3
    logits = rng.integers(-4, 3, (N, C)).astype(np.float32) if integer else rng.standard_normal((N, C)).astype(np.float32)
    known = (gt >= 0) & (gt < C)
    boost = known & (rng.random(N) < 0.8)
    logits[boost, gt[boost]] += np.float32(5 if integer else 4.5)
    tie = np.flatnonzero(known)[:: max(1, N // 12)]                      # a tie at the top: the lowest index wins
    logits[tie] = np.float32(-1)
    logits[tie, gt[tie]] = 2
    logits[tie, (gt[tie] + 1) % C] = 2
    if integer:
        features = rng.integers(-3, 4, (N, F)).astype(np.float32)
    else:
        centres = 3 * rng.standard_normal((C + 4, F))
        features = (centres[np.clip(gt, 0, C + 3)] + rng.standard_normal((N, F)) * (1 + rng.random((N, 1)))).astype(np.float32)
    nan_row = int(np.flatnonzero(boost)[0]) if boost.any() else 0
    logits[nan_row, C // 2] = np.nan
    return features, logits, gt.astype(np.int64)


def make_tail_case(N, C, seed):
    """(dist fp32 [N], gt, correct uint8 [N]) for the fit alone. By class index modulo 5: 0 = quantised distances (ties, also across
    the tail boundary), 1 = no correct row, 2 = one correct row, 3 = all distances equal, 4 = plain. Distances lie in [5, 10]
    (relative spread of a tail >= 1e-3 by far); a NaN and a +Inf sit on correct rows of class 0; labels -1, -2, C, C + 2 appear."""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, C, N)
    odd = rng.random(N)
    gt[odd < 0.05] = -1
    gt[(odd >= 0.05) & (odd < 0.08)] = -2
    gt[(odd >= 0.08) & (odd < 0.11)] = C
    gt[(odd >= 0.11) & (odd < 0.13)] = C + 2
    correct = (rng.random(N) < 0.8) | (gt == 0)
    dist = (5 + 5 * rng.random(N)).astype(np.float32)
    role = np.where((gt >= 0) & (gt < C), gt % 5, -1)
    dist[role == 0] = np.round(dist[role == 0] * 4) / 4
    correct[role == 1] = False
    one = np.flatnonzero(role == 2)
    correct[one[1:]] = False
    if len(one):
        correct[one[0]] = True
    dist[role == 3] = np.float32(7.5)
    zero = np.flatnonzero(gt == 0)                                        # all correct
    order = zero[np.argsort(dist[zero], kind="stable")]
    dist[order[-1]] += np.float32(0.125)                                 # one largest value,
    dist[order[-3]] = dist[order[-2]]                                    # ties across the boundary of a tail of 2
    if len(order) > 21:
        dist[order[-21]] = dist[order[-20]]                              # ... and of 20
    dist[order[0]], dist[order[1]] = np.nan, np.inf
    return dist, gt.astype(np.int64), correct.astype(np.uint8)


def ulp_jitter(d, rng):
    """d moved by -1, 0 or +1 fp32 ulp at random (finite entries)."""
    d = np.asarray(d, dtype=np.float32)
    step = rng.integers(-1, 2, d.shape)
    out = np.where(step > 0, np.nextafter(d, np.float32(np.inf)), np.where(step < 0, np.nextafter(d, np.float32(-np.inf)), d))
    return np.where(np.isfinite(d), out, d).astype(np.float32)


def jitter_movement(features, logits, gt, T, metric, alpha, seeds=range(5)):
    """The largest movement of the oracle's own probs when the fp32 distances of fit and of predict move by +-1 ulp at random."""
    mav, _, correct = class_means(features, logits, gt)
    d_fit, d_all = distances(features, mav, gt, metric), distances(features, mav, None, metric)
    base = fit_tails(d_fit, gt, correct, len(mav), T)
    p0 = predict(base, logits, features, alpha, metric, dist=d_all)
    worst = 0.0
    for s in seeds:
        rng = np.random.default_rng(1000 + s)
        m = fit_tails(ulp_jitter(d_fit, rng), gt, correct, len(mav), T)
        p = predict(m, logits, features, alpha, metric, dist=ulp_jitter(d_all, rng))
        worst = max(worst, float(np.nanmax(np.abs(p.astype(np.float64) - p0))))
    return worst

"""numpy fp64 restatement of activation shaping as include/osi.h (ABI 27) defines it: the canonical order, exact order statistics, the
kept set of a row, the five shaping modes, numpy's `linear` percentile and the three logit scores. Nothing here is fast; it is what the
GPU tests compare against (tests/test_shaping_gpu.py) and what tests/test_shaping_cpu.py checks on hand-worked rows."""
import numpy as np

REACT, ASH_P, ASH_B, ASH_S, SCALE = 0, 1, 2, 3, 4
ENERGY, MAXLOGIT, MSP = 0, 1, 2
MODES = {"react": REACT, "ash_p": ASH_P, "ash_b": ASH_B, "ash_s": ASH_S, "scale": SCALE}
MAX_R, MAX_F = 8, 4096


def canonical(v):
    """The value the order compares: v + 0.0f in fp32 (-0 becomes +0)."""
    return np.asarray(v, dtype=np.float32) + np.float32(0.0)


def ascending(v):
    """Indices of v (1-D) in the ascending canonical order: IEEE order, every NaN after +Inf; a stable sort on (isnan, value)."""
    c = canonical(v)
    nan = np.isnan(c)
    return np.lexsort((np.where(nan, np.float32(0.0), c), nan))          # the LAST key is the primary one; lexsort is stable


def order_stats(v, ranks):
    """The ranks[r]-th element, 0-based and ascending, of the values v (any shape): their canonical values, fp32."""
    c = canonical(v).ravel()
    return c[ascending(c)[np.asarray(ranks, dtype=np.int64)]]


def keep_of(width, percentile):
    """The rule of the ASH code."""
    return int(width) - int(np.round(int(width) * percentile / 100.0))


def kept_set(row, keep):
    """Boolean mask [F]: the first `keep` columns of the row in descending canonical order, NaN first, ties by ascending column."""
    c = canonical(row)
    nan = np.isnan(c)
    order = np.lexsort((-np.where(nan, np.float32(0.0), c).astype(np.float64), ~nan))     # stable: equal values stay in column order
    mask = np.zeros(len(c), dtype=bool)
    mask[order[:keep]] = True
    return mask


def kept_masks(x, keep):
    """kept_set of every row: [M, F]."""
    return np.stack([kept_set(row, keep) for row in np.asarray(x, dtype=np.float32)])


def shape_rows(x, mode, keep=0, clip=0.0, kept=None):
    """out [M, F] fp32 and the kept masks [M, F] (all True for REACT and SCALE). Sums and the exponential in fp64, one rounding to fp32,
    one fp32 product - the arithmetic of the definition, summed in numpy's order. `kept`: kept_masks(x, keep) where the caller has them."""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty_like(x)
    masks = np.ones(x.shape, dtype=bool)
    if mode == REACT:
        assert keep == 0
        c = np.float32(clip)
        with np.errstate(invalid="ignore"):
            return np.where(x > c, c, x), masks
    assert 1 <= keep <= x.shape[1]
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for i, row in enumerate(x):
            k = kept_set(row, keep) if kept is None else kept[i]
            s1, s2 = row.astype(np.float64).sum(), row[k].astype(np.float64).sum()
            if mode == ASH_P:
                out[i] = np.where(k, row, zero)
            elif mode == ASH_B:
                out[i] = np.where(k, np.float32(s1 / keep), zero)
            else:
                scaled = row * np.float32(np.exp(s1 / s2))                # fp32 * fp32 -> fp32
                out[i] = scaled if mode == SCALE else np.where(k, scaled, zero)
            if mode != SCALE:
                masks[i] = k
    return out, masks


def linear_percentile(values, percentile):
    """numpy's `linear` rule on the canonical order, in fp64: h = (n - 1) p / 100, j = floor(h), a + (h - j)(b - a). Returns
    (value, j, n)."""
    c = canonical(values).ravel()
    n = c.size
    h = (n - 1) * (percentile / 100.0)
    j = int(np.floor(h))
    a, b = (float(t) for t in order_stats(c, [j, min(j + 1, n - 1)]))
    return a + (h - j) * (b - a), j, n


def logit_scores(logits, mode):
    """[M] fp64: log-sum-exp, largest logit or largest softmax probability; an infinite maximum is not subtracted, a NaN in a row
    makes the row's result NaN."""
    lg = np.asarray(logits, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(lg, axis=1)
        shift = np.where(np.isfinite(m), m, 0.0)
        s = np.exp(lg - shift[:, None]).sum(axis=1)
        if mode == ENERGY:
            return shift + np.log(s)
        if mode == MAXLOGIT:
            return np.where(np.isnan(s), np.nan, m)
        return np.exp(m - shift) / s


def head(x, fc_weight, fc_bias, logit_weight, logit_bias=None):
    """The two head layers in fp64."""
    f = np.asarray(x, np.float64) @ np.asarray(fc_weight, np.float64).T + np.asarray(fc_bias, np.float64)
    lg = f @ np.asarray(logit_weight, np.float64).T
    return lg if logit_bias is None else lg + np.asarray(logit_bias, np.float64)


def ulps(a, b):
    """Distance in fp32 units in the last place between two fp32 arrays; 0 where both are NaN, a huge number where one is."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)

    def ordered(v):
        i = (v + np.float32(0.0)).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)

    d = np.abs(ordered(a) - ordered(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, 1 << 40, d))


# ---- the inputs of the GPU tests, shared with the CPU tests that check the oracle on them ------------------------------------------
def relu_rows(m, f, seed):
    """ReLU-like rows: about half exact zeros (ties cross every cut), row 0 all equal where there is one to spare, duplicated values."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((m, f)), 0.0).astype(np.float32)
    x[rng.random((m, f)) < 0.25] = np.float32(0.75)           # duplicates at whatever value becomes the threshold
    if m > 1:
        x[0] = np.float32(1.25)
    return x


def stats_data(name, n, seed=0):
    rng = np.random.default_rng(seed + n)
    if name == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if name == "ties":
        return rng.integers(0, 4, n).astype(np.float32)
    if name == "equal":
        return np.full(n, -2.5, dtype=np.float32)
    if name == "denormal":
        return (rng.integers(-50, 50, n).astype(np.float32) * np.float32(1e-45)).astype(np.float32)
    assert name == "special"
    v = rng.standard_normal(n).astype(np.float32)
    pick = rng.random(n)
    for lo, value in ((0.0, 0.0), (0.1, -0.0), (0.2, np.inf), (0.25, -np.inf), (0.3, np.nan)):
        v[(pick >= lo) & (pick < lo + 0.05)] = value
    return v


STATS_DATA = ("normal", "ties", "equal", "denormal", "special")

"""numpy restatement of the deep-nearest-neighbour selection as include/osi.h (ABI 24) defines it: the order (canonical value d + 0,
every NaN after +Inf, ties by ascending column, one skipped column per row), osi_knn_topk, osi_knn_class_kth and its three transforms,
the latter evaluated in np.float32 step by step. A helper of tests/test_knn_cpu.py and tests/test_knn_gpu.py, not collected as a test.
Selection does no arithmetic, so everything here is exact: the GPU tests ask for equal bits."""
import numpy as np

RAW, SIM_COSINE, SIM_INVERSE = 0, 1, 2
MAX_K = 1024


def canonical(d):
    """d + 0.0f: -0 becomes +0, everything else keeps its bits (a NaN stays a NaN)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(d, dtype=np.float32) + np.float32(0)


def sort_key(v):
    """fp64 key of canonical values whose numeric order is the defined one: NaN mapped behind +Inf (as a rank, not a value)."""
    v = np.asarray(v, dtype=np.float32)
    key = v.astype(np.float64)
    # ranks: finite and -Inf as they are, +Inf stays +Inf, NaN must come later still: order by (is_nan, value)
    return np.isnan(v), np.where(np.isnan(v), 0.0, key)


def order(row, skip=-1):
    """The columns of one row in the defined order, the skipped one left out."""
    v = canonical(row)
    nan, key = sort_key(v)
    cols = np.arange(len(v))
    perm = np.lexsort((cols, key, nan))                  # last key is the primary one: NaN flag, then value, then column
    if 0 <= skip < len(v):
        perm = perm[perm != skip]
    return perm, v


def topk(dist, N, K, skip=None):
    """(out_dist [M, K] fp32, out_idx [M, K] int64) from dist [M, ld >= N]: +Inf / -1 past min(K, n)."""
    dist = np.asarray(dist, dtype=np.float32)[:, :N]
    M = len(dist)
    out_d = np.full((M, K), np.inf, dtype=np.float32)
    out_i = np.full((M, K), -1, dtype=np.int64)
    for m in range(M):
        perm, v = order(dist[m], -1 if skip is None else int(skip[m]))
        n = min(K, len(perm))
        out_d[m, :n] = v[perm[:n]]
        out_i[m, :n] = perm[:n]
    return out_d, out_i


def transform(v, what):
    """What osi_knn_class_kth stores for the selected value v (fp32 array), every operation rounded to fp32."""
    v = np.asarray(v, dtype=np.float32)
    if what == RAW:
        return v.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if what == SIM_COSINE:
            t = np.float32(0.5) * v
            s = np.float32(1) - t
            out = np.minimum(np.maximum(s, np.float32(0)), np.float32(1)).astype(np.float32)
        elif what == SIM_INVERSE:
            out = (np.float32(1) / (np.float32(1) + v)).astype(np.float32)
        else:
            raise ValueError(what)
    return np.where(np.isnan(v), np.float32(np.nan), out).astype(np.float32)


def class_kth(dist, N, start, K, skip=None, what=RAW):
    """out [M, C] fp32 from dist [M, ld >= N] and start [C + 1] (clamped to [0, N]; a descending pair is an empty class)."""
    dist = np.asarray(dist, dtype=np.float32)[:, :N]
    start = np.clip(np.asarray(start).astype(np.int64), 0, N)
    M, C = len(dist), len(start) - 1
    out = np.full((M, C), np.inf, dtype=np.float32)
    for m in range(M):
        sk = -1 if skip is None else int(skip[m])
        for c in range(C):
            c0, c1 = int(start[c]), int(start[c + 1])
            if c1 <= c0:
                continue
            perm, v = order(dist[m, c0:c1], sk - c0 if c0 <= sk < c1 else -1)
            if len(perm):
                out[m, c] = v[perm[min(K, len(perm)) - 1]]
    return transform(out, what)


def same_values(a, b):
    """Bit-equal where not NaN, NaN in the same places (a NaN's payload is not part of the definition)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b))) and \
        bool(np.array_equal(np.where(nan, np.float32(0), a).view(np.uint32), np.where(nan, np.float32(0), b).view(np.uint32)))

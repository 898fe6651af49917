"""numpy fp64 restatement of the two kernels of include/osi.h (ABI 29) - the head of ODIN and GradNorm for the last linear layer -, the
literal textbook ODIN on a torch model, and the grid search of ODIN.tune. Nothing here is fast; it is what tests/test_odin_gpu.py and
tests/test_odin_cpu.py compare against. A plain module, imported like the other oracles."""
import numpy as np
import torch

from shaping_oracle import ulps  # noqa: F401  (the fp32 ulp distance the tests read from here)


def argmax_rows(logits):
    """torch.argmax per row: a NaN counts as the largest value, the lowest index wins among equals (numpy's rule as well)."""
    return np.argmax(np.asarray(logits), axis=1).astype(np.int64)


def _exponentials(logits, T):
    lg = np.asarray(logits, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(lg, axis=1)
        shift = np.where(np.isfinite(m), m, 0.0)
        return np.exp((lg - shift[:, None]) / float(T))


def odin_head(logits, T):
    """(dlogits [M, C], pred [M], score [M]) in fp64: e = exp((l - m') / T), r = the sum of e without the predicted column,
    s = e_y + r, score = e_y / s, dlogits = e / s and -r / s in the predicted column."""
    pred = argmax_rows(logits)
    e = _exponentials(logits, T)
    rows = np.arange(len(e))
    with np.errstate(all="ignore"):
        e_y = e[rows, pred]
        rest = e.copy()
        rest[rows, pred] = 0.0
        r = rest.sum(axis=1)
        s = e_y + r
        d = e / s[:, None]
        d[rows, pred] = -r / s
        return d, pred, e_y / s


def gradnorm(features, logits, T):
    """[M] fp64: ||f||_1 * sum_c |C p_c - 1| / T, p = softmax(logits / T) under the same shift."""
    e = _exponentials(logits, T)
    with np.errstate(all="ignore"):
        p = e / e.sum(axis=1)[:, None]
        c = e.shape[1]
        return np.abs(np.asarray(features, dtype=np.float64)).sum(axis=1) * np.abs(c * p - 1.0).sum(axis=1) / float(T)


def gradnorm_bound(features, logits, T, want):
    """The bound of the GPU test: one fp32 rounding of the result plus the fp64 error of the near-uniform rows, where the terms
    |C p_c - 1| cancel and the error is absolute: ||f||_1 C (C + 4) 2^-52 / T (every p_c differs by at most (C + 4) 2^-53 relative
    between two fp64 evaluations)."""
    c = np.asarray(logits).shape[1]
    l1 = np.abs(np.asarray(features, dtype=np.float64)).sum(axis=1)
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + l1 * c * (c + 4) * 2.0 ** -52 / float(T)


# ---- the literal method on a torch model that returns (logits, features) ------------------------------------------------------------
def textbook_loss(logits, T):
    """J per row: -log max softmax(z / T)."""
    return -torch.log(torch.softmax(logits / T, 1).max(1).values)


def textbook_odin(model, x, T, epsilon, lo=0.0, hi=1.0):
    """(x~, image gradient, unknown): g = autograd.grad of the summed -log max softmax(z / T), x~ = clamp(x - epsilon sign(g)),
    unknown = -max softmax(model(x~) / T)."""
    xi = x.detach().clone().requires_grad_()
    logits, _ = model(xi)
    g, = torch.autograd.grad(textbook_loss(logits, T).sum(), xi)
    x_t = torch.clamp(x.detach() - epsilon * torch.sign(g), lo, hi)
    with torch.no_grad():
        logits_t, _ = model(x_t)
        unknown = -torch.softmax(logits_t / T, 1).max(1).values
    return x_t, g, unknown


def pick(rows):
    """The grid point ODIN.tune selects from rows of (T, epsilon, fpr95, auroc, ...): the lowest FPR at 95 % TPR, then the higher
    AUROC, then the smaller T, then the smaller epsilon - a plain loop."""
    best = None
    for row in rows:
        key = (row[2], -row[3], row[0], row[1])
        if best is None or key < best[0]:
            best = (key, row)
    return best[1]


def tune(model, batches, temperatures, epsilons, unk_label, detection_metrics):
    """Brute force over the grid with textbook_odin: the rows (T, epsilon, fpr95, auroc, aupr_in, aupr_out), T-major."""
    gt = np.concatenate([np.asarray(y) for _, y in batches]).astype(np.int64)
    rows = []
    for T in temperatures:
        for eps in epsilons:
            u = np.concatenate([textbook_odin(model, x, T, eps)[2].numpy() for x, _ in batches])
            m = detection_metrics(gt, u, unk_label=unk_label, tpr=(0.95,))
            rows.append([float(T), float(eps), m["fpr_at_tpr"][0], m["auroc"], m["aupr_in"], m["aupr_out"]])
    return rows


# ---- the rows of the GPU tests --------------------------------------------------------------------------------------------------------
def head_rows(m, c, seed):
    """[m, c] fp32 logits for the head's test. Row 0 (always): the maximum duplicated in two columns owned by different lanes (c >= 66)
    or wherever two columns exist; row 1: duplicated inside one lane's columns (the quad form: columns of one quad; the ragged form:
    columns 64 apart, where the row has them); row 2: one dominant logit (p_y >= 1 - 1e-10 at T <= 1); row 3: all equal. The rest are normal draws times 3."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((m, c))).astype(np.float32)
    top = np.float32(20.0)
    if c >= 2:
        x[0, [c - 1, c // 2]] = top                            # different lanes (or at least different columns), the lower index wins
    if m > 1 and c >= 3:
        quad = c % 4 == 0 and c <= 1024
        a = 4 * (c // 8) if quad else 1                         # the quad form: columns a + 1, a + 3 of one quad
        pair = [a + 1, a + 3] if quad else ([0, 64] if c > 64 else [1, 2])
        x[1, pair] = top
    if m > 2:
        x[2] = (rng.standard_normal(c)).astype(np.float32)
        x[2, c // 3] = np.float32(40.0)                         # a gap of 36 or more: nonzero in fp32 at T = 0.5 still
    if m > 3:
        x[3] = np.float32(-0.75)
    return x

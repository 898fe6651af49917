"""fp64 numpy restatement of PROSER as include/osi.h (ABI 23) defines it: the pairwise mix (with the exact fp32 emulation of its
formula), the three-term loss and its gradients, the scores and the bias calibration. Test infrastructure only."""
import math

import numpy as np


# ---- the mix ---------------------------------------------------------------------------------------------------------------------------
def fma_f32(a, b, c):
    """fmaf(a, b, c) on fp32 arrays, correctly rounded: a * b is exact in fp64 (24 + 24 bits); its sum with c is rounded TO ODD in
    fp64 (TwoSum gives the error of the rounded sum; where it is not zero and the sum's last bit is even, the neighbour on the error's
    side is the odd one), and a round-to-odd value of 53 >= 2 * 24 + 2 bits rounds to fp32 as the exact sum would."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        q = np.broadcast_to(c.astype(np.float64), p.shape)
        s = p + q
        bb = s - p
        e = (p - (s - bb)) + (q - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        # towards the error: up when e has the sign that increases s
        s_odd = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s_odd.astype(np.float32)


def mix_row_f32(w, x, y):
    """x' = fmaf(w, x, (1 - w) * y) in fp32: 1 - w rounded once, the product rounded once, then the fma."""
    w = np.float32(w)
    with np.errstate(all="ignore"):
        omw = np.float32(np.float32(1.0) - w)
        t = (omw * np.asarray(y, dtype=np.float32)).astype(np.float32)
    return fma_f32(np.full_like(np.asarray(x, dtype=np.float32), w), x, t)


def mix_rows_pairs_f32(x, partner, weight):
    """The bits osi_mix_rows_pairs leaves for an involution `partner`: x [B, L] fp32 -> a new array."""
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    B = x.shape[0]
    for i in range(B):
        j = int(partner[i])
        if j <= i or j >= B:          # itself, out of range, or written by its owner
            continue
        out[i] = mix_row_f32(weight[i], x[i], x[j])
        out[j] = mix_row_f32(weight[j], x[j], x[i])
    return out


def mix_rows_pairs_f64(x, partner, weight):
    x = np.asarray(x, dtype=np.float64)
    out = x.copy()
    B = x.shape[0]
    for i in range(B):
        j = int(partner[i])
        if 0 <= j < B and j != i:
            out[i] = float(weight[i]) * x[i] + (1.0 - float(weight[i])) * x[j]
    return out


def is_involution(partner):
    partner = np.asarray(partner)
    idx = np.arange(len(partner))
    return bool(((partner >= 0) & (partner < len(partner))).all() and (partner[partner] == idx).all())


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def first_argmax(row):
    """First index of the largest entry; a NaN counts as largest (torch.max)."""
    row = np.asarray(row, dtype=np.float64)
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def _lse(v):
    v = np.asarray(v, dtype=np.float64)
    if np.isnan(v).any():
        return float("nan")
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def loss_and_grads(logits, dummy, target, n_mixed, lambdas):
    """(loss4 = [J, mean t1, mean t2, mean t3], dlogits [B, C], ddummy [B, D]) in fp64."""
    z = np.asarray(logits, dtype=np.float64)
    d = np.asarray(dummy, dtype=np.float64)
    y = np.asarray(target, dtype=np.int64)
    B, C = z.shape
    l0, l1, l2 = (float(v) for v in lambdas)
    n1 = int(n_mixed)
    clean = [i for i in range(n1, B) if 0 <= y[i] < C]
    n2 = len(clean)
    dz, dd = np.zeros_like(z), np.zeros_like(d)
    t1 = t2 = t3 = 0.0
    with np.errstate(all="ignore"):
        for i in list(range(n1)) + clean:
            a = first_argmax(d[i])
            e = np.concatenate([z[i], d[i, a:a + 1]])
            lse = _lse(e)
            s = np.exp(e - lse)
            if i < n1:
                t1 += lse - e[C]
                g = s.copy()
                g[C] -= 1.0
                g *= l0 / n1
            else:
                yi = int(y[i])
                rest = np.delete(e, yi)
                lse2 = _lse(rest)
                t2 += lse - e[yi]
                t3 += lse2 - e[C]
                s2 = np.exp(e - lse2)
                s2[yi] = 0.0
                g1 = s.copy()
                g1[yi] -= 1.0
                g2 = s2
                g2[C] -= 1.0
                g = l1 / n2 * g1 + l2 / n2 * g2
            dz[i] = g[:C]
            dd[i, a] = g[C]
    m1 = t1 / n1 if n1 else 0.0
    m2 = t2 / n2 if n2 else 0.0
    m3 = t3 / n2 if n2 else 0.0
    J = (l0 * m1 if n1 else 0.0) + (l1 * m2 if n2 else 0.0) + (l2 * m3 if n2 else 0.0)
    return np.array([J, m1, m2, m3]), dz, dd


def torch_loss(logits, dummy, target, n_mixed, lambdas, minus_1e9=False):
    """The plainly written formula in torch, in the dtype of `logits` (differentiable): (J, [J, m1, m2, m3]). minus_1e9: the third term
    as the published implementations write it (e_y = -1e9) instead of leaving the column out."""
    import torch
    import torch.nn.functional as F
    B, C = logits.shape
    m = dummy.max(dim=1, keepdim=True).values
    e = torch.cat([logits, m], dim=1)
    zero = e.sum() * 0
    n1 = int(n_mixed)
    clean = torch.tensor([i for i in range(n1, B) if 0 <= int(target[i]) < C], dtype=torch.long)
    unk = torch.full((n1,), C, dtype=torch.long)
    m1 = F.cross_entropy(e[:n1], unk) if n1 else zero
    if len(clean):
        ec, yc = e[clean], target[clean].long()
        m2 = F.cross_entropy(ec, yc)
        if minus_1e9:
            masked = ec.clone()
            masked[torch.arange(len(clean)), yc] = -1e9
            m3 = F.cross_entropy(masked, torch.full((len(clean),), C, dtype=torch.long))
        else:
            keep = torch.ones_like(ec, dtype=torch.bool)
            keep[torch.arange(len(clean)), yc] = False
            rest = ec[keep].view(len(clean), C)            # column y left out; the placeholder is the last of the C that stay
            m3 = F.cross_entropy(rest, torch.full((len(clean),), C - 1, dtype=torch.long))
    else:
        m2 = m3 = zero
    l0, l1, l2 = lambdas
    J = (l0 * m1 if n1 else zero) + (l1 * m2 if len(clean) else zero) + (l2 * m3 if len(clean) else zero)
    return J, torch.stack([J, m1, m2, m3])


# ---- scores and bias -------------------------------------------------------------------------------------------------------------------
def scores(logits, dummy, bias):
    z = np.asarray(logits, dtype=np.float64)
    d = np.asarray(dummy, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(d).any(axis=1), np.nan, d.max(axis=1)) + float(bias)
        e = np.concatenate([z, m[:, None]], axis=1)
        e = e - np.where(np.isnan(e).any(axis=1), np.nan, e.max(axis=1))[:, None]
        p = np.exp(e)
        return p / p.sum(axis=1, keepdims=True)


def bias_index(n, known_rate):
    return min(int(math.floor((1.0 - known_rate) * n)), n - 1)


def fit_bias(logits, dummy, gt, known_rate=0.95):
    """The floor((1 - known_rate) * n)-th smallest (0-based) of delta = max_c logits - max_d dummy over the rows with 0 <= gt < C; the
    differences are taken in fp32, as the device takes them."""
    z = np.asarray(logits, dtype=np.float32)
    d = np.asarray(dummy, dtype=np.float32)
    y = np.asarray(gt).astype(np.int64)
    known = (y >= 0) & (y < z.shape[1])
    delta = np.sort((z.max(axis=1) - d.max(axis=1))[known])
    return float(delta[bias_index(len(delta), known_rate)])

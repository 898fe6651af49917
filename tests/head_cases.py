"""Inputs, label batches and float64 references of the head and pooling kernel tests. TEST INFRASTRUCTURE ONLY.

tests/test_head_kernels_gpu.py runs the HIP kernels on these cases; tests/test_head_reference_cpu.py shows, without a kernel, that the
references below are right (oracle == torch.nn.CrossEntropyLoss == boolean-mask indexing) and that every label batch holds the kinds of
row its case claims. All references are plain torch on the CPU in float64.
"""
import torch
import torch.nn.functional as F

from oracle import losses_oracle as LO

ENTROPIC, SOFTMAX, GARBAGE = 0, 1, 2          # OSI_LOSS_* of include/osi.h
MODES = {"entropic": ENTROPIC, "softmax": SOFTMAX, "garbage": GARBAGE}
LOSS_WAVES = 16                               # k_loss / k_confidence: rows i, i + 16, ... belong to one wave
LOSS_MAX_B = 15 * 1024                        # lse[B] lives in LDS

# (B, C, logit scale, label kind). B around the 16 waves and at the LDS limit; C around the 64 lanes; C = 5 only at the limit.
LOSS_SHAPES = [(B, C, 3.0, "mixed") for B in (1, 15, 16, 17, 40) for C in (1, 64, 65, 130)] + [
    (LOSS_MAX_B, 5, 3.0, "mixed"),
    (17, 65, 40.0, "mixed"),                  # large-magnitude logits
    (40, 65, 3.0, "last_row_known"),          # the only known row is row 39: wave 7, third trip
]


def loss_id(case):
    B, C, scale, kind = case
    return f"B{B}-C{C}-x{int(scale)}-{kind}"


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def logits(B, C, scale, g):
    return torch.randn(B, C, generator=g) * scale


def class_weights(C, g, zeros="some"):
    """fp32 class weights U[0.5, 1.5); "some": every third class has weight exactly 0 (never all of them)."""
    cw = torch.rand(C, generator=g) + 0.5
    if zeros == "some" and C > 1:
        cw[1::3] = 0
    return cw


def labels(mode, B, C, kind, g, ignore_index=-1):
    """(y, claims): an int64 label batch of one loss mode and the kinds of row it is built to contain.
    claims = {"known": n, "unknown": n, "ignored": n}: minimum counts, checked by the CPU test through row_kinds().
      entropic  knowns, -1 and -2 (every negative label is an unknown)
      softmax   knowns and ignore_index (-1, or a class index: then every label is a class index, as torch requires)
      garbage   knowns, -100 and -1 (neither is a class: no term, no weight)"""
    y = torch.randint(0, C, (B,), generator=g)
    claims = {"known": 0, "unknown": 0, "ignored": 0}
    if kind == "last_row_known":
        y[:] = {ENTROPIC: -1, SOFTMAX: ignore_index, GARBAGE: -100}[mode]
        y[B - 1] = (ignore_index + 1) % C if mode == SOFTMAX and ignore_index >= 0 else C // 2
        claims["known"] = 1
        claims["unknown" if mode == ENTROPIC else "ignored"] = 1
        return y, claims
    assert kind == "mixed"
    if B < 3:                                 # a single row: one known label
        if mode == SOFTMAX and ignore_index >= 0 and C > 1:
            y[y == ignore_index] = (ignore_index + 1) % C
        if mode == GARBAGE:
            y[y % 3 == 1] -= 1                # class_weights() gives the classes 1, 4, 7, ... weight 0: a lone row of one is 0 / 0
        claims["known"] = int(not (mode == SOFTMAX and ignore_index >= 0 and C == 1))
        claims["ignored"] = 1 - claims["known"]
        return y, claims
    # a third of the rows (and always rows 1, 2 and the last but one) carry the mode's non-class labels
    odd = torch.rand(B, generator=g) < 0.33
    odd[1] = odd[2] = odd[B - 2] = True
    odd[0] = odd[B - 1] = False
    n = int(odd.sum())
    if mode == ENTROPIC:
        neg = torch.where(torch.rand(n, generator=g) < 0.5, -1, -2)
        neg[0], neg[1] = -1, -2
        y[odd] = neg
        claims.update(known=1, unknown=2)
    elif mode == SOFTMAX:
        if ignore_index >= 0 and C > 1:
            y[y == ignore_index] = (ignore_index + 1) % C
        y[odd] = ignore_index
        claims.update(known=int(C > 1 or ignore_index < 0), ignored=1)
    else:
        neg = torch.where(torch.rand(n, generator=g) < 0.5, -100, -1)
        neg[0], neg[1] = -100, -1
        y[odd] = neg
        claims.update(known=1, ignored=2)
    return y, claims


def row_kinds(mode, y, C, ignore_index=-1):
    """What the kernel's contract makes of each row: (known, unknown, ignored) boolean masks. A label >= C is ignored everywhere."""
    in_range = (y >= 0) & (y < C)
    if mode == ENTROPIC:
        return in_range, y < 0, y >= C
    if mode == SOFTMAX:
        known = in_range & (y != ignore_index)
        return known, torch.zeros_like(known), ~known
    return in_range, torch.zeros_like(in_range), ~in_range


def normaliser(mode, y, C, cw=None, ignore_index=-1):
    """The batch quantity the loss divides by: B (entropic), the count of used rows (softmax), the sum of their weights (garbage)."""
    known = row_kinds(mode, y, C, ignore_index)[0]
    if mode == ENTROPIC:
        return float(y.shape[0])
    if mode == SOFTMAX:
        return float(known.sum())
    return float(cw.double()[y[known]].sum())


def loss_ref64(mode, z, y, w=1.0, cw=None, ignore_index=-1, masked=False):
    """(J, dJ/dz) in float64 from torch.nn.CrossEntropyLoss. masked=False hands torch the whole batch, the way the reference calls
    it (entropic: soft targets; softmax: ignore_index=...; garbage: weight=..., torch's default ignore_index=-100 drops a -100
    label). masked=True selects the used rows with a boolean mask first (labels torch would refuse: -1 in garbage mode, y >= C in any
    mode) and keeps the mode's divisor: the rows left out get no loss term and, through autograd, an all-zero gradient row."""
    z64 = z.double().clone().requires_grad_(True)
    B, C = z.shape
    if mode == ENTROPIC:
        if masked:
            keep = y < C
            t = LO.entropic_targets(y[keep], C, w, torch.float64)
            J = torch.nn.CrossEntropyLoss(reduction="sum")(z64[keep], t) / B
        else:
            J = torch.nn.CrossEntropyLoss()(z64, LO.entropic_targets(y, C, w, torch.float64))
    elif mode == SOFTMAX:
        if masked:
            keep = (y >= 0) & (y < C) & (y != ignore_index)
            J = torch.nn.CrossEntropyLoss()(z64[keep], y[keep])
        else:
            J = torch.nn.CrossEntropyLoss(ignore_index=ignore_index)(z64, y)
    else:
        if masked:
            keep = (y >= 0) & (y < C)
            J = torch.nn.CrossEntropyLoss(weight=cw.double())(z64[keep], y[keep])
        else:
            J = torch.nn.CrossEntropyLoss(weight=cw.double())(z64, y)
    J.backward()
    return J.detach(), z64.grad


def needs_mask(mode, y, C):
    """Does the batch hold a label torch.nn.CrossEntropyLoss refuses in this mode?"""
    if mode == ENTROPIC:
        return bool((y >= C).any())
    if mode == SOFTMAX:
        return bool(((y < -1) | (y >= C)).any())
    return bool((((y < 0) & (y != -100)) | (y >= C)).any())


def oracle_loss64(mode, z64, y, w=1.0, cw=None, ignore_index=-1):
    """The oracle's restatement on the rows selected by boolean-mask indexing, with the mode's divisor (float64, differentiable)."""
    B, C = z64.shape
    known, unknown, _ = row_kinds(mode, y, C, ignore_index)
    if mode == ENTROPIC:
        keep = known | unknown
        return LO.entropic_openset_loss(z64[keep], y[keep], w) * (float(keep.sum()) / B)
    if mode == SOFTMAX:
        return LO.softmax_loss(z64[known], y[known], ignore_index=-1)
    return LO.garbage_loss(z64[known], y[known], cw.double())


def entropic_closed_form64(z, y, w):
    """dJ/dz of the entropic loss with the rows y >= C removed and the divisor B: (s_i p - t_i) / B on the
    rows kept, exactly 0 on the rows removed."""
    B, C = z.shape
    keep = y < C
    t = torch.zeros(B, C, dtype=torch.float64)
    t[keep] = LO.entropic_targets(y[keep], C, w, torch.float64)
    return (t.sum(1, keepdim=True) * torch.softmax(z.double(), 1) - t) / B


def with_labels_past_the_end(y, C):
    """Rows 0 and the last but two relabelled C and C + 7 (a first-trip row and, from B = 19, a later-trip one). Returns (y, rows)."""
    y = y.clone()
    rows = sorted({0, max(0, y.shape[0] - 3)})
    for k, r in enumerate(rows):
        y[r] = C + 7 * k
    return y, rows


def loss_case(mode, case):
    """(z, y, cw, claims) of one entry of LOSS_SHAPES in one mode."""
    B, C, scale, kind = case
    g = gen(mode, B, C, int(scale), len(kind))
    z = logits(B, C, scale, g)
    y, claims = labels(mode, B, C, kind, g)
    return z, y, class_weights(C, g) if mode == GARBAGE else None, claims


def softmax_ignore_cases():
    """(id, z, y, ignore_index, claims): ignore_index -1, 0 and C - 1 (the latter two on class-index labels only, as torch requires),
    and the batches with every row ignored (torch: 0 / 0 = NaN)."""
    out = []
    for B, C in ((17, 65), (40, 130)):
        for ii in (-1, 0, C - 1):
            g = gen(11, B, C, ii + 1)
            y, claims = labels(SOFTMAX, B, C, "mixed", g, ii)
            out.append((f"B{B}-C{C}-ignore{ii}", logits(B, C, 3.0, g), y, ii, claims))
    g = gen(12)
    out.append(("B17-C65-all-ignored", logits(17, 65, 3.0, g), torch.full((17,), -1), -1, {"known": 0, "unknown": 0, "ignored": 17}))
    out.append(("B16-C1-ignore0-all-ignored", logits(16, 1, 3.0, g), torch.zeros(16, dtype=torch.int64), 0, {"known": 0, "unknown": 0, "ignored": 16}))
    return out


def garbage_cases():
    """(id, z, y, cw, claims), every batch one torch.nn.CrossEntropyLoss(weight=cw) takes whole: a -100 label (ignored, torch's
    default ignore_index), weights with zeros, and a batch whose present classes all have weight 0 (torch: 0 / 0 = NaN)."""
    out = []
    for name, B, C, zeros in (("minus100", 17, 65, "none"), ("zero-weights", 40, 130, "some")):
        g = gen(13, B, C)
        y = torch.randint(0, C, (B,), generator=g)
        y[1] = y[B - 2] = -100
        if zeros == "some":
            y[0], y[B - 1] = 1, 2                         # class 1 has weight 0, class 2 has not
        out.append((f"B{B}-C{C}-{name}", logits(B, C, 3.0, g), y, class_weights(C, g, zeros), {"known": 2, "unknown": 0, "ignored": 2}))
    g = gen(14)
    B, C = 17, 65
    cw = class_weights(C, g, "some")
    y = torch.randint(0, 21, (B,), generator=g) * 3 + 1   # classes 1, 4, 7, ...: all of weight 0
    y[3] = -100
    out.append(("B17-C65-present-classes-weigh-0", logits(B, C, 3.0, g), y, cw, {"known": 1, "unknown": 0, "ignored": 1}))
    return out


# ---- objectosphere ---------------------------------------------------------------------------------------------------------------
# (B, C, F): F != C everywhere. The first nine have F > C; the last two F < C.
OBJECTO_SHAPES = [(B, {5: 3, 64: 5, 130: 65}[Fd], Fd) for B in (16, 17, 40) for Fd in (5, 64, 130)] + [(17, 65, 5), (40, 130, 64)]
OBJECTO_PARAMS = ((10.0, 1e-2, 1.0), (3.0, 0.5, 0.5))       # (xi, alpha, unknown weight)
ROW_ZERO, ROW_OUTSIDE, ROW_INSIDE, ROW_UNKNOWN = 0, 1, 2, 3  # planted rows; the same four kinds again in the last four rows


def objecto_case(B, C, Fd, xi, g):
    """(z, y, f): f[ROW_ZERO] = 0 (gradient defined as 0), a known row with |f| = 2 xi (residual 0: dfeat exactly 0), a known row with
    |f| = xi / 2, an unknown row; B > 16 plants the same kinds in rows B-4 .. B-1, which belong to a later trip of their waves."""
    z = torch.randn(B, C, generator=g) * 2
    y = torch.randint(-1, C, (B,), generator=g)
    f = torch.randn(B, Fd, generator=g) * 3
    for base in ((0,) if B <= 16 else (0, B - 4)):
        y[base + ROW_ZERO] = 0 if base == 0 else -1
        f[base + ROW_ZERO] = 0
        y[base + ROW_OUTSIDE] = C - 1
        f[base + ROW_OUTSIDE] *= 2 * xi / f[base + ROW_OUTSIDE].norm()
        y[base + ROW_INSIDE] = 0
        f[base + ROW_INSIDE] *= 0.5 * xi / f[base + ROW_INSIDE].norm()
        y[base + ROW_UNKNOWN] = -1
    return z, y, f


def objecto_ref64(z, y, f, w, xi, alpha):
    z64, f64 = z.double().requires_grad_(True), f.double().requires_grad_(True)
    J = LO.objectosphere_loss(z64, y, f64, w, xi, alpha)
    J.backward()
    return J.detach(), z64.grad, f64.grad


# ---- confidence ------------------------------------------------------------------------------------------------------------------
CONF_SHAPES = [(B, C) for B in (17, 40) for C in (65, 151)]


def conf_last_valid(C):
    return (None, -1, 64, 65, C)


def conf_case(B, C, unknown_class, g):
    """(scores fp32, y): softmax scores whose unknown rows (label unknown_class) peak at column 64, at column 65 (if there is one)
    and at column C - 1, so that every cut scores[:, :last_valid_class] of the test drops some row's maximum; labels hold knowns,
    unknowns and -2 rows (counted on neither side)."""
    z = torch.randn(B, C, generator=g) * 2
    y = torch.randint(0, C - 1, (B,), generator=g)            # knowns: never the class C - 1, which may stand for "unknown"
    y[torch.rand(B, generator=g) < 0.25] = unknown_class
    y[torch.rand(B, generator=g) < 0.2] = -2
    y[0], y[4] = 3, -2
    if B > LOSS_WAVES + 1:
        y[LOSS_WAVES] = 5                                     # a known row in a later trip of its wave (B = 17: row 16 is the unknown below)
    for row, col in ((1, 64), (2, min(65, C - 1)), (3, C - 1), (B - 1, 64)):
        y[row] = unknown_class
        z[row, col] = 10.0                                      # N(0, 2^2) elsewhere: the row's maximum
    return torch.softmax(z, 1), y


# ---- softmax ---------------------------------------------------------------------------------------------------------------------
SOFTMAX_SHAPES = [(1, 1), (5, 64), (6, 65), (37, 151), (9, 1000)]


def softmax_case(B, C, g):
    """N(0, 4^2) logits; from three rows on: row 0 alternates +80 / -80, row 1 holds -inf in every third column, row 2 is constant."""
    z = torch.randn(B, C, generator=g) * 4
    if B >= 3:
        z[0] = 80.0
        z[0, 1::2] = -80.0
        z[1, ::3] = float("-inf")
        z[2] = -7.25
    return z


# ---- linear ----------------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(11, 116, 116), (9, 152, 152), (3, 260, 9), (8, 4, 1), (1, 2048, 8)]


def linear_case(B, K, O, g):
    x, w, b = torch.randn(B, K, generator=g), torch.randn(O, K, generator=g) / K ** .5, torch.randn(O, generator=g)
    dy = torch.randn(B, O, generator=g)
    return x, w, b, dy


def linear_ref(x, w, b, dy, dt):
    """(y, dx, dw, db) of F.linear by autograd in dtype dt; b None = no bias."""
    xx, ww = (t.to(dt).clone().requires_grad_(True) for t in (x, w))
    bb = None if b is None else b.to(dt).clone().requires_grad_(True)
    y = F.linear(xx, ww, bb)
    y.backward(dy.to(dt))
    return y.detach(), xx.grad, ww.grad, None if b is None else bb.grad


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
MAXPOOL_SHAPES = [(2, 4, 7, 12), (1, 8, 2, 2), (2, 64, 15, 16), (1, 4, 1, 5)]
MAXPOOL_INPUTS = ("randn", "negative", "relu")


def maxpool_case(B, C, H, W, kind, g):
    """(x, dy) NCHW fp32. "randn" has negatives, "negative" is -rand - 1 (every value <= -1: zero padding would win every border
    window), "relu" is post-ReLU (many exact ties at 0). dy lies on a grid of 1/64 with |dy| <= 4: every sum of up to four of them is
    exact in fp32, so the backward comparison carries no rounding at all."""
    x = torch.randn(B, C, H, W, generator=g)
    if kind == "negative":
        x = -torch.rand(B, C, H, W, generator=g) - 1
    elif kind == "relu":
        x = F.relu(x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randint(-256, 257, (B, C, Ho, Wo), generator=g).float() / 64
    return x, dy


def maxpool_ref(x, dy, dt=torch.float64):
    xx = x.to(dt).clone().requires_grad_(True)
    y = F.max_pool2d(xx, 3, 2, 1)
    y.backward(dy.to(dt))
    return y.detach(), xx.grad


AVGPOOL_SHAPES = [(3, HW, C) for HW in (1, 4, 9, 16, 50) for C in (4, 2048)]


def avgpool_case(B, HW, C, g):
    """(x [B, HW, C], dy [B, C]) fp32, the kernel's own layout."""
    return torch.randn(B, HW, C, generator=g), torch.randn(B, C, generator=g)


def avgpool_ref64(x, dy):
    xx = x.double().clone().requires_grad_(True)
    y = xx.mean(dim=1)
    y.backward(dy.double())
    return y.detach(), xx.grad

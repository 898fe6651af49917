"""Cases and float64 references of the non-finite propagation tests. TEST INFRASTRUCTURE ONLY.

The contract (include/osi.h, conventions; DESIGN.md, divergences): given the same non-finite inputs, the SET of non-finite output
elements of every entry point equals that of the torch reference of the same operation, and every finite element stays within the
bound the parity test of that entry point uses. NaN versus +-Inf is not asserted.

tests/test_nonfinite_gpu.py runs the HIP kernels on these cases; tests/test_nonfinite_cpu.py shows without a kernel that every
reference below gives the same mask in fp32 and fp64, that each case contaminates what it claims ("partial": some but not all
elements, "none": nothing, "all": the listed outputs entirely) and that no case rests on a non-finite value times a structural zero
(padding taps, rows past M), which the contract leaves unspecified.

A case is a small record: the shape, which operand is poisoned with which value at which element, and `expect`. The references
are plain torch on the CPU; `dt` selects float32 or float64.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

NAN, INF = float("nan"), float("inf")
VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF}


def nonfinite(t):
    return ~torch.isfinite(t)


def masks_equal(a, b):
    return torch.equal(nonfinite(a), nonfinite(b))


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------
# forward: one element of channel C0 of y poisoned. backward: clean forward, one element of dout poisoned, at an element whose
# ReLU gate is open / closed (picked from the fp64 forward with a margin of 0.1, so that fp32 and the kernels agree on it).
BnCase = namedtuple("BnCase", "B C H relu res operand value gate expect")
BN_SHAPES = [(5, 12, 6), (3, 256, 7), (2, 64, 56)]          # rows form, 16-channel groups past one block, many row blocks
BN_FORMS = [(True, False), (True, True), (False, False)]    # (relu, res) as in test_batchnorm
BN_C0 = 5
BN_CASES = [BnCase(B, C, H, relu, res, "y", v, None, "partial") for B, C, H in BN_SHAPES for relu, res in BN_FORMS for v in ("nan", "+inf")]
BN_CASES += [BnCase(B, C, H, relu, res, "dout", v, gate, "partial" if gate == "open" else "none")
             for B, C, H in BN_SHAPES for relu, res in BN_FORMS for v in ("nan", "+inf")
             for gate in (("open", "closed") if relu else ("open",))]


def bn_id(c):
    return f"B{c.B}-C{c.C}-H{c.H}-{'relu' if c.relu else 'lin'}{'-res' if c.res else ''}-{c.operand}-{c.value}" + (f"-{c.gate}" if c.gate else "")


def bn_inputs(c):
    """The draws of test_batchnorm (same seed, same order), then the poison."""
    import osi_testlib as T
    g = torch.Generator().manual_seed(c.C + c.H)
    y = torch.randn(c.B, c.C, c.H, c.H, generator=g) * 2 + torch.randn(1, c.C, 1, 1, generator=g) * 5
    gamma, beta = T.bn_state(c.C, g, "positive")
    rm0, rv0 = torch.randn(c.C, generator=g), torch.rand(c.C, generator=g) + 0.5
    resid = torch.randn(c.B, c.C, c.H, c.H, generator=g) if c.res else None
    dout = torch.randn(c.B, c.C, c.H, c.H, generator=g)
    d = dict(y=y, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, resid=resid, dout=dout)
    if c.operand == "y":
        d["at"] = (c.B - 1, BN_C0, c.H // 2, c.H - 1)
        y[d["at"]] = VALUES[c.value]
    else:
        pre = F.batch_norm(y.double(), None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)
        if c.res:
            pre = pre + resid.double()
        ch = pre[:, BN_C0]
        want = (ch > 0.1) if c.gate == "open" else (ch < -0.1)
        b, h, w = [int(v) for v in want.nonzero()[-1]]       # the last such element: not in the first row block
        d["at"] = (b, BN_C0, h, w)
        d["pre_at"] = float(ch[b, h, w])
        dout[d["at"]] = VALUES[c.value]
    return d


def bn_ref(c, d, dt):
    """dict of every output of the BatchNorm entry points, NCHW / [C], by autograd in dtype dt."""
    yy = d["y"].to(dt).clone().requires_grad_(True)
    ga, be = d["gamma"].to(dt).clone().requires_grad_(True), d["beta"].to(dt).clone().requires_grad_(True)
    rm, rv = d["rm0"].to(dt).clone(), d["rv0"].to(dt).clone()
    o = F.batch_norm(yy, rm, rv, ga, be, True, 0.1, 1e-5)
    if c.res:
        o = o + d["resid"].to(dt)
    if c.relu:
        o = F.relu(o)
    o.backward(d["dout"].to(dt))
    y = d["y"].to(dt)
    mean = y.mean(dim=(0, 2, 3))
    var = y.var(dim=(0, 2, 3), unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    scale = d["gamma"].to(dt) * invstd
    gate = (o.detach() > 0) if c.relu else torch.ones_like(o, dtype=torch.bool)
    gm = torch.where(gate, d["dout"].to(dt), torch.zeros((), dtype=dt))      # a select, like torch's threshold_backward
    return dict(out=o.detach(), mean=mean, invstd=invstd, scale=scale, shift=d["beta"].to(dt) - mean * scale, running_mean=rm,
                running_var=rv, dy=yy.grad, dgamma=ga.grad, dbeta=be.grad, gm=gm)


BN_FWD_OUTPUTS = ("out", "mean", "invstd", "scale", "shift", "running_mean", "running_var")
BN_BWD_OUTPUTS = ("dy", "dgamma", "dbeta", "gm")


def channel_of(name, t, c0):
    """(the part of output `name` that belongs to channel c0, the rest)."""
    if t.dim() == 1:
        keep = torch.ones(t.numel(), dtype=torch.bool); keep[c0] = False
        return t[c0:c0 + 1], t[keep]
    keep = torch.ones(t.shape[1], dtype=torch.bool); keep[c0] = False
    return t[:, c0], t[:, keep]


# ---- convolution epilogue statistics ---------------------------------------------------------------------------------------------
BnStatsCase = namedtuple("BnStatsCase", "Cin Cout k stride H B value expect")
BNSTATS_CASES = [BnStatsCase(64, 64, 1, 1, 14, 3, "nan", "all"), BnStatsCase(64, 64, 1, 1, 56, 3, "nan", "all")]
BNSTATS_FORMS = ((128, 2048), (1, 2048), (1, 0))          # (bn_single_p, bn_wide_p): rows, wide, two-level (as _conv_bnstats_case)
BNSTATS_TILES = (0, 4, 5, 2)


def bnstats_inputs(c):
    """The draws of _conv_bnstats_case; one NaN input pixel (every input channel of it would do; one is the hard case)."""
    g = torch.Generator().manual_seed(c.Cin + c.Cout + c.H)
    x = torch.randn(c.B, c.Cin, c.H, c.H, generator=g) + 0.3
    w = torch.randn(c.Cout, c.Cin, c.k, c.k, generator=g) / (c.Cin * c.k * c.k) ** 0.5
    at = (1, 7, c.H // 2, c.H // 3)
    x[at] = VALUES[c.value]
    return dict(x=x, w=w, at=at, g=g)


def bnstats_ref(c, d, dt):
    y = F.conv2d(d["x"].to(dt), d["w"].to(dt), None, c.stride, 0)
    rm, rv = torch.zeros(c.Cout, dtype=dt), torch.ones(c.Cout, dtype=dt)
    F.batch_norm(y, rm, rv, None, None, True, 0.1, 1e-5)
    mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    return dict(mean=mean, invstd=invstd, scale=invstd, shift=-mean * invstd, running_mean=rm, running_var=rv)


# ---- convolutions ----------------------------------------------------------------------------------------------------------------
# op: fwd (x or w poisoned), dgrad (dy), wgrad (dy or x). where: "interior" (image 1, centre), "corner" (image 0, pixel (0, 0)),
# "last" (the last pixel of the last image: the ragged row tile), "odd" (pixel (1, 1) of a stride-2 1x1 layer: read by nothing),
# "filter" (a whole filter w[K0]).
ConvCase = namedtuple("ConvCase", "Cin Cout k stride pad H B op operand where value expect")
CONV_SHAPES = [(64, 64, 3, 1, 1, 7), (128, 128, 3, 2, 1, 9), (64, 128, 1, 2, 0, 7), (64, 64, 1, 1, 0, 9)]
CONV_C0, CONV_K0 = 9, 17


def _conv_cases(shapes, wino=False):
    out = []
    for Cin, Cout, k, stride, pad, H, B in shapes:
        s = (Cin, Cout, k, stride, pad, H, B)
        for where in ("interior", "corner", "last"):
            for v in (("nan", "+inf") if where == "interior" else ("nan",)):
                out.append(ConvCase(*s, "fwd", "x", where, v, "partial"))
                out.append(ConvCase(*s, "dgrad", "dy", where, v, "partial"))
                # weight gradient, padded: a poisoned dy next to the border meets padding taps, a poisoned x next to it the dy rows
                # outside the image (0 * NaN: unspecified); the Winograd form F(3x3, 2x2) spreads a border x over those taps (NaN - NaN)
                if pad == 0 or where == "interior":
                    out.append(ConvCase(*s, "wgrad", "dy", where, v, "partial"))
                    out.append(ConvCase(*s, "wgrad", "x", where, v, "partial"))
        out.append(ConvCase(*s, "fwd", "w", "filter", "nan", "partial"))
        if k == 1 and stride == 2:
            out.append(ConvCase(*s, "fwd", "x", "odd", "nan", "none"))
            out.append(ConvCase(*s, "wgrad", "x", "odd", "nan", "none"))
    return out


CONV_CASES = _conv_cases([s + (3,) for s in CONV_SHAPES])
# (B, H, W, Cin, Cout) of the Winograd forms, 3x3 stride 1 pad 1
WINO_SHAPES = [(6, 7, 7, 64, 128), (5, 10, 6, 64, 64)]
WinoCase = namedtuple("WinoCase", "B H W Cin Cout op operand where value expect")
WINO_CASES = [WinoCase(B, H, W, Cin, Cout, c.op, c.operand, c.where, c.value, c.expect)
              for B, H, W, Cin, Cout in WINO_SHAPES for c in _conv_cases([(Cin, Cout, 3, 1, 1, H, B)], wino=True)]
SPLITK_CASE = ConvCase(64, 64, 3, 1, 1, 56, 2, "wgrad", "dy", "interior", "nan", "partial")


def conv_id(c):
    shape = "-".join(str(v) for v in c[:-5])
    return f"{shape}-{c.op}-{c.operand}-{c.where}-{c.value}"


def poison_at(where, B, C, H, W, c0):
    """NCHW index of the poisoned element of a [B][C][H][W] tensor."""
    return {"interior": (1, c0, H // 2, W // 2), "corner": (0, c0, 0, 0), "last": (B - 1, c0, H - 1, W - 1), "odd": (1, c0, 1, 1)}[where]


def conv_inputs(c, W=None):
    """The draws of test_conv_fwd_dgrad_wgrad (x, w, dy in NCHW / OIHW), then the poison. W: image width (default H)."""
    W = c.H if W is None else W
    k, stride, pad = (c.k, c.stride, c.pad) if hasattr(c, "k") else (3, 1, 1)
    g = torch.Generator().manual_seed(c.Cin * 7 + c.Cout + k + c.H)
    x = torch.randn(c.B, c.Cin, c.H, W, generator=g)
    w = torch.randn(c.Cout, c.Cin, k, k, generator=g) / (c.Cin * k * k) ** 0.5
    Ho, Wo = (c.H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn(c.B, c.Cout, Ho, Wo, generator=g)
    base = torch.randn(c.B, c.H, W, c.Cin, generator=g)
    v = VALUES[c.value]
    at = None
    if c.operand == "x":
        at = poison_at(c.where, c.B, c.Cin, c.H, W, CONV_C0)
        if c.where == "interior":                                # a pixel a strided 1x1 layer reads
            at = at[:2] + (at[2] // stride * stride, at[3] // stride * stride)
        x[at] = v
    elif c.operand == "dy":
        at = poison_at(c.where, c.B, c.Cout, Ho, Wo, CONV_K0)
        dy[at] = v
    else:
        w[CONV_K0] = v
    return dict(x=x, w=w, dy=dy, base=base, at=at, k=k, stride=stride, pad=pad)


def conv_ref(c, d, dt):
    x, w, dy, s, p = d["x"].to(dt), d["w"].to(dt), d["dy"].to(dt), d["stride"], d["pad"]
    if c.op == "fwd":
        return dict(y=F.conv2d(x, w, None, s, p))
    if c.op == "dgrad":
        dx = torch.nn.grad.conv2d_input(x.shape, w, dy, s, p)
        return dict(dx=dx, dx_acc=dx + d["base"].to(dt).permute(0, 3, 1, 2))
    return dict(dw=torch.nn.grad.conv2d_weight(x, w.shape, dy, s, p))


def conv_taps_inside(d, Hin, Win):
    """Does the poisoned dy element see all k*k taps inside the image? (weight-gradient cases on padded layers must)"""
    _, _, ho, wo = d["at"]
    k, s, p = d["k"], d["stride"], d["pad"]
    return 0 <= ho * s - p and ho * s - p + k - 1 < Hin and 0 <= wo * s - p and wo * s - p + k - 1 < Win


# ---- fused-activation loaders ----------------------------------------------------------------------------------------------------
# the A operand is relu(x * scale + shift) [+ res]; poisons: one NaN element of x in a channel of positive scale, and a NaN shift
# (a whole NaN channel: what a diverged BatchNorm hands the next layer)
ActCase = namedtuple("ActCase", "entry Cin Cout k stride H B operand expect")
def _act_expect(entry, op):
    """a NaN shift makes every activation of the channel NaN: every output of a forward, one input-channel slice of a weight gradient"""
    return "all" if op == "shift" and not entry.startswith("wgrad") else "partial"


_ACT = [(e, 64, 64, 1, 1, 14, 3, op) for e in ("fwd_act", "wgrad_act", "fwd_rows") for op in ("x", "shift")]
_ACT += [(e, 64, 128, 3, 1, 9, 3, op) for e in ("fwd_act", "wgrad_act") for op in ("x", "shift")]           # the row-window forms
_ACT += [(e, 128, 64, 3, 2, 9, 2, op) for e in ("fwd_act", "wgrad_act") for op in ("x", "shift")]           # stride 2: parity classes
_ACT += [("fwd_act2", 256, 64, 1, 1, 14, 3, op) for op in ("x", "shift", "res")]
_ACT += [(e, 64, 128, 3, 1, 7, 6, op) for e in ("fwd_wino", "wgrad_wino") for op in ("x", "shift")]
ACT_CASES = [ActCase(*a, _act_expect(a[0], a[-1])) for a in _ACT]
ACT_C0 = 6


def act_id(c):
    return f"{c.entry}-{c.Cin}-{c.Cout}-k{c.k}-H{c.H}-B{c.B}-{c.operand}"


def act_inputs(c):
    """x NHWC, scale / shift (the positive state), w [Cout][k][k][Cin], dy NHWC, res (fwd_act2); then the poison."""
    import osi_testlib as T
    g = torch.Generator().manual_seed(c.Cin * 7 + c.Cout + c.k + c.H)
    x = torch.randn(c.B, c.H, c.H, c.Cin, generator=g) * 1.5
    sc, sh = T.bn_state(c.Cin, g, "positive", beta_std=0.7)
    w = torch.randn(c.Cout, c.k, c.k, c.Cin, generator=g) / (c.Cin * c.k * c.k) ** 0.5
    Ho = (c.H + 2 * (c.k // 2) - c.k) // c.stride + 1
    dy = torch.randn(c.B, Ho, Ho, c.Cout, generator=g)
    res = torch.relu(torch.randn(c.B, c.H, c.H, c.Cin, generator=g)) if c.entry == "fwd_act2" else None
    at = (1, c.H // 2, c.H // 2, ACT_C0)
    if c.operand == "x":
        x[at] = NAN
    elif c.operand == "res":
        res[at] = NAN
    else:
        sh[ACT_C0] = NAN
    assert float(sc[ACT_C0]) > 0
    return dict(x=x, sc=sc, sh=sh, w=w, dy=dy, res=res, at=at)


def act_ref(c, d, dt):
    """NHWC / [Cout][k][k][Cin] outputs of conv(relu(x * scale + shift) [+ res], w) resp. its weight gradient."""
    a = torch.relu(d["x"].to(dt) * d["sc"].to(dt) + d["sh"].to(dt))
    if d["res"] is not None:
        a = torch.relu(d["x"].to(dt) * d["sc"].to(dt) + d["sh"].to(dt) + d["res"].to(dt))
    a, w, pad = a.permute(0, 3, 1, 2), d["w"].to(dt).permute(0, 3, 1, 2), c.k // 2
    if c.entry.startswith("wgrad"):
        return dict(dw=torch.nn.grad.conv2d_weight(a, w.shape, d["dy"].to(dt).permute(0, 3, 1, 2), c.stride, pad).permute(0, 2, 3, 1))
    return dict(y=F.conv2d(a, w, None, c.stride, pad).permute(0, 2, 3, 1))


# ---- inference epilogues ---------------------------------------------------------------------------------------------------------
EpiCase = namedtuple("EpiCase", "B H Cin Cout k relu shortcut operand expect")
EPI_CASES = [EpiCase(B, H, Cin, Cout, k, relu, sc, op, "partial")
             for B, H, Cin, Cout, k in ((5, 9, 64, 192, 1), (8, 28, 128, 128, 3)) for relu in (True, False) for sc in (False, True)
             for op in (("x", "scale", "res") if sc else ("x", "scale"))]
EPI_WINO_CASES = [EpiCase(8, 28, 128, 128, 3, relu, False, op, "partial") for relu in (True, False) for op in ("x", "scale")]
EPI_IMAGE, EPI_N0 = 2, 11


def epi_id(c):
    return f"B{c.B}-H{c.H}-{c.Cin}-{c.Cout}-k{c.k}-{'relu' if c.relu else 'lin'}{'-shortcut' if c.shortcut else ''}-{c.operand}"


def epi_inputs(c):
    """(clean, poisoned) operand dicts: x NHWC (post-ReLU: non-negative), w [Cout][k][k][Cin], scale, shift, res [M][Cout]."""
    g = torch.Generator().manual_seed(c.B * 1000 + c.H * 10 + c.k)
    x = torch.rand(c.B, c.H, c.H, c.Cin, generator=g)
    w = torch.randn(c.Cout, c.k, c.k, c.Cin, generator=g) / (c.Cin * c.k * c.k) ** 0.5
    sc, sh = torch.rand(c.Cout, generator=g) + 0.5, torch.randn(c.Cout, generator=g) * 0.3
    res = torch.randn(c.B * c.H * c.H, c.Cout, generator=g) if c.shortcut else None
    clean = dict(x=x, w=w, sc=sc, sh=sh, res=res)
    bad = {k: (None if v is None else v.clone()) for k, v in clean.items()}
    if c.operand == "x":
        bad["x"][EPI_IMAGE, c.H // 2, c.H // 2, 3] = NAN
    elif c.operand == "scale":
        bad["sc"][EPI_N0] = NAN
    else:
        bad["res"][(EPI_IMAGE * c.H + c.H // 2) * c.H + 1, EPI_N0] = NAN
    return clean, bad


def epi_ref(c, d, dt):
    """[B][H][H][Cout] of [relu](conv(x, w) * scale + shift [+ res])."""
    y = F.conv2d(d["x"].to(dt).permute(0, 3, 1, 2), d["w"].to(dt).permute(0, 3, 1, 2), None, 1, c.k // 2).permute(0, 2, 3, 1)
    y = y * d["sc"].to(dt) + d["sh"].to(dt)
    if c.shortcut:
        y = y + d["res"].to(dt).view(y.shape)
    return dict(out=torch.relu(y) if c.relu else y)


# ---- pools -----------------------------------------------------------------------------------------------------------------------
PoolCase = namedtuple("PoolCase", "B H W C fused value expect")
POOL_CASES = [PoolCase(B, H, W, C, fused, v, "none" if (v == "-inf") else "partial")
              for B, H, W, C in ((2, 17, 23, 64), (4, 9, 9, 8)) for fused in (False, True) for v in ("nan", "+inf", "-inf")]
POOL_POISONS = ("interior", "corner", "last")       # every case poisons these three elements (different channels)


def pool_id(c):
    return f"B{c.B}-{c.H}x{c.W}-C{c.C}-{'bn_relu_maxpool' if c.fused else 'maxpool'}-{c.value}"


def pool_inputs(c):
    """x NCHW (fused: the pre-BN tensor, with scale / shift of positive scale), dy on a grid of 1/64 (sums of four exact in fp32)."""
    g = torch.Generator().manual_seed(c.B + c.H * 3 + c.W * 5 + c.C)
    x = torch.randn(c.B, c.C, c.H, c.W, generator=g)
    sc, sh = torch.rand(c.C, generator=g) + 0.5, torch.randn(c.C, generator=g) * 0.5
    Ho, Wo = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    dy = torch.randint(-256, 257, (c.B, c.C, Ho, Wo), generator=g).float() / 64
    at = [poison_at(wh, c.B, c.C, c.H, c.W, c0) for wh, c0 in zip(POOL_POISONS, (1, 2, 7))]
    for a in at:
        x[a] = VALUES[c.value]
    return dict(x=x, sc=sc, sh=sh, dy=dy, at=at)


def pool_ref(c, d, dt):
    x = d["x"].to(dt)
    if c.fused:
        x = torch.relu(x * d["sc"].to(dt).view(1, -1, 1, 1) + d["sh"].to(dt).view(1, -1, 1, 1))
    xx = x.clone().requires_grad_(True)
    y, idx = F.max_pool2d(xx, 3, 2, 1, return_indices=True)
    y.backward(d["dy"].to(dt))
    return dict(y=y.detach(), idx=idx, dx=xx.grad, act=x)


def avgpool_linear_inputs(which):
    import head_cases as H
    if which == "avgpool":
        x, dy = H.avgpool_case(3, 9, 2048, H.gen(71))
        x[1, 4, 33] = NAN
        dy = dy.clone(); dy[2, 5] = NAN
        return dict(x=x, dy=dy)
    x, w, b, dy = H.linear_case(9, 152, 152, H.gen(72))
    x[3, 17] = NAN
    return dict(x=x, w=w, b=b, dy=dy)


def avgpool_linear_ref(which, d, dt):
    import head_cases as H
    if which == "avgpool":
        xx = d["x"].to(dt).clone().requires_grad_(True)
        y = xx.mean(dim=1)
        y.backward(d["dy"].to(dt))
        return dict(y=y.detach(), dx=xx.grad)
    y, dx, dw, db = H.linear_ref(d["x"], d["w"], d["b"], d["dy"], dt)
    return dict(y=y, dx=dx, dw=dw, db=db)


# ---- head ------------------------------------------------------------------------------------------------------------------------
# row: "counted" (a row with a loss term), "ignored" (a row torch.nn.CrossEntropyLoss itself ignores: ignore_index / -100; softmax and
# garbage modes), "refused" (a label >= C, which torch refuses: the reference takes the row out before the loss, head_cases.loss_ref64)
LossCase = namedtuple("LossCase", "mode row value expect")
LOSS_B, LOSS_C = 17, 65
LOSS_CASES = [LossCase(m, "counted", v, "partial") for m in ("entropic", "softmax", "garbage") for v in ("nan", "+inf")]
LOSS_CASES += [LossCase(m, "ignored", v, "partial") for m in ("softmax", "garbage") for v in ("nan", "+inf")]
LOSS_CASES += [LossCase(m, "refused", "nan", "none") for m in ("entropic", "softmax", "garbage")]


def loss_id(c):
    return f"{c.mode}-{c.row}-{c.value}"


def loss_inputs(c):
    import head_cases as H
    m = H.MODES[c.mode]
    z, y, cw, _ = H.loss_case(m, (LOSS_B, LOSS_C, 3.0, "mixed"))
    if cw is not None:
        cw = torch.rand(LOSS_C, generator=H.gen(73)) + 0.5      # no zero weights: a counted row has a term
    known, unknown, ignored = H.row_kinds(m, y, LOSS_C)
    if c.row == "counted":
        row = int(known.nonzero()[-1])                         # row 16: the second trip of wave 0
    elif c.row == "ignored":
        row = int(ignored.nonzero()[0])
        if m == H.GARBAGE:
            y[row] = -100
    else:
        row = int(known.nonzero()[0])
        y[row] = LOSS_C + 3
    z[row, 40] = VALUES[c.value]
    return dict(z=z, y=y, cw=cw, row=row, mode=m)


def loss_ref(c, d, dt):
    """(loss, dlogits) in dtype dt; torch.nn.CrossEntropyLoss on the whole batch, or on the batch without the refused rows."""
    import head_cases as H
    m, z, y, cw = d["mode"], d["z"], d["y"], d["cw"]
    zz = z.to(dt).clone().requires_grad_(True)
    from oracle import losses_oracle as LO
    in_range = (y >= 0) & (y < LOSS_C)
    keep = {H.ENTROPIC: y < LOSS_C, H.SOFTMAX: in_range | (y == -1), H.GARBAGE: in_range | (y == -100)}[m]      # the labels torch accepts
    if m == H.ENTROPIC:
        J = torch.nn.CrossEntropyLoss(reduction="sum")(zz[keep], LO.entropic_targets(y[keep], LOSS_C, 1.0, dt)) / LOSS_B
    elif m == H.SOFTMAX:
        J = torch.nn.CrossEntropyLoss(ignore_index=-1)(zz[keep], y[keep])
    else:
        J = torch.nn.CrossEntropyLoss(weight=cw.to(dt))(zz[keep], y[keep])
    J.backward()
    return dict(loss=J.detach(), dz=zz.grad)


OBJECTO_ROWS = ("known", "unknown")
OBJECTO_F, OBJECTO_XI, OBJECTO_ALPHA = 5, 3.0, 0.5


def objecto_inputs(row_kind):
    """Entropic loss + objectosphere term on (17, 65) logits and 5-dimensional features (no all-zero feature row: its gradient is
    defined as 0 here and 0 / 0 in torch); one NaN feature element in the last known / unknown row."""
    import head_cases as H
    g = H.gen(76)
    z, y, _, _ = H.loss_case(H.ENTROPIC, (LOSS_B, LOSS_C, 3.0, "mixed"))
    f = torch.randn(LOSS_B, OBJECTO_F, generator=g) * 3
    row = int(((y >= 0) if row_kind == "known" else (y < 0)).nonzero()[-1])
    f[row, 2] = NAN
    return dict(z=z, y=y, f=f, row=row)


def objecto_ref(d, dt):
    from oracle import losses_oracle as LO
    zz, ff = d["z"].to(dt).clone().requires_grad_(True), d["f"].to(dt).clone().requires_grad_(True)
    J = LO.objectosphere_loss(zz, d["y"], ff, 1.0, OBJECTO_XI, OBJECTO_ALPHA)
    J.backward()
    return dict(loss=J.detach(), dz=zz.grad, df=ff.grad)


def softmax_inputs():
    import head_cases as H
    z = H.softmax_case(6, 65, H.gen(74))
    z[3, 64] = NAN
    z[4, 7] = INF
    return z


def conf_inputs(row_kind, form):
    """(scores or logits, y, offset, unknown_class): a NaN in a known row ("known") or in a row labelled unknown ("negative")."""
    import head_cases as H
    scores, y = H.conf_case(17, 65, -1, H.gen(75))
    arg = scores if form == "scores" else torch.log(scores)
    row = int(((y >= 0) if row_kind == "known" else (y == -1)).nonzero()[-1])
    arg = arg.clone()
    arg[row, int(y[row]) if row_kind == "known" else 12] = NAN
    return arg, y, 1.0 / 65, -1, row


def conf_ref(arg, y, offset, unknown_class, form, dt):
    """The four accumulators as oracle.losses_oracle.confidence states them (sums, not means), on scores in dtype dt."""
    s = arg.to(dt) if form == "scores" else torch.softmax(arg.to(dt), 1)
    known, neg = (y >= 0) & (y != unknown_class), y == unknown_class
    ks = s[known, y[known]].sum()
    ns = (1 + offset - torch.max(s[neg], dim=1)[0]).sum()
    return torch.stack([ks, torch.tensor(float(known.sum()), dtype=dt), ns, torch.tensor(float(neg.sum()), dtype=dt)])


# ---- whole network ---------------------------------------------------------------------------------------------------------------
NET_POISONS = ("pixel", "filter")
NET_FILTER_KEY, NET_FILTER = "resnet_base.layer3.0.conv2.weight", 5


def network_inputs(poison, image=1):
    """tests/osi_testlib.py's geometry on the positive BatchNorm state (B = 4, 64 x 64, C = 10), then the poison."""
    import osi_testlib as T
    from oracle import resnet50_oracle as R
    gen = torch.Generator().manual_seed(47)
    sd = R.init_state(T.NET_C, T.NET_C, False, generator=gen)
    R.randomize_bn(sd, generator=gen)
    x = torch.rand(T.NET_B, 3, T.NET_HW, T.NET_HW, generator=gen)
    y = torch.randint(-1, T.NET_C, (T.NET_B,), generator=gen)
    clean = x.clone()
    if poison == "pixel":
        x[image, 1, 30, 31] = NAN
    else:
        sd[NET_FILTER_KEY][NET_FILTER] = NAN
    return sd, x, y, clean

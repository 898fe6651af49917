"""GPU: the frozen-statistics BatchNorm backward (ABI 12). Per kernel through the C ABI against torch-CPU fp64 at the project's
per-kernel bound (2e-6 + 6e-8 sqrt(K)) max|ref| (tests/test_input_grad_gpu.py), every case on the positive and the signed BatchNorm
state; then the whole network: eval-mode gradients, freeze_bn(), the input-only form, FGSM in eval mode, staged calls, state errors."""
import ctypes
import functools
import math

import pytest
import torch

from openset_imagenet import _native as N

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-4        # the project's rel-L2 bar of the 162 parameter gradients: the frozen bar may never exceed it
EPS = 1e-5


def _bound(K, ref):
    return (2e-6 + 6e-8 * math.sqrt(K)) * float(ref.abs().max())


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _frozen_bn(C, gen, kind):
    """A BatchNorm on frozen statistics: (gamma, beta, mean, invstd, scale, shift), fp32 on the CPU; scale / shift as the coefficient
    kernels form them (gamma * invstd, beta - mean * scale)."""
    import osi_testlib as T
    gamma, beta = T.bn_state(C, gen, kind)
    mean = 0.1 * torch.randn(C, generator=gen)
    invstd = 1.0 / torch.sqrt(0.5 + torch.rand(C, generator=gen) + EPS)
    scale = gamma * invstd
    return gamma, beta, mean, invstd, scale, beta - mean * scale


# ---- 3. frozen in-block input gradient -------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, k, stride, cus): cus > 0 forces a K-split tail the way tests/test_tail_split_gpu.py does (knob "tail_cus")
DGRAD_CASES = [(3, 9, 11, 128, 64, 1, 1, 0),        # 1x1, M = 297: a ragged row tile
               (2, 10, 12, 64, 64, 3, 1, 0),        # 3x3 stride 1: the row-window form
               (2, 13, 15, 64, 64, 3, 2, 0),        # 3x3 stride 2: parity classes
               (2, 12, 12, 128, 64, 3, 1, 9),       # row windows + K-split tail + fix-up
               (3, 14, 14, 64, 128, 1, 1, 4)]       # 1x1 + K-split tail + fix-up


@pytest.mark.parametrize("kind", ["positive", "signed"])
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,cus", DGRAD_CASES)
def test_frozen_inblock_dgrad_vs_fp64(cuda, B, H, W, Cin, Cout, k, stride, cus, kind):
    import osi_testlib as T
    L = N.lib()
    pad = 1 if k == 3 else 0
    gen = torch.Generator().manual_seed(1000 * Cin + 10 * H + k + stride + (7 if kind == "signed" else 0))
    d = N.ConvDesc.make(B, H, W, Cin, Cout, k, stride, pad)
    M = B * H * W
    dy = torch.randn(B, d.Ho, d.Wo, Cout, generator=gen)
    w = torch.randn(Cout, k, k, Cin, generator=gen) / (Cout * k * k) ** 0.5
    y0 = torch.randn(M, Cin, generator=gen) * 2 + 0.5
    gamma, beta, mean, invstd, scale, shift = _frozen_bn(Cin, gen, kind)
    dev = lambda t: t.contiguous().to(cuda)
    dy_d, w_d, y0_d, mean_d, inv_d, sc_d, sh_d = map(dev, (dy, w, y0, mean, invstd, scale, shift))
    gate = (torch.addcmul(sh_d, y0_d, sc_d) > 0).cpu()                           # the fma the kernels evaluate
    if kind == "signed":
        assert float((0.05 * invstd * (y0 - mean).abs().max(0).values).max()) < 1.0      # classes 4 / 5 saturate the gate
        T.assert_signed_gates(gate, Cin, "recomputed gate")

    def run(pb, with_partials=True):
        parts = torch.full((max(pb, 16) // 4,), float("nan"), device=cuda)
        f = T.Fusion(y0=y0_d.data_ptr(), mean0=mean_d.data_ptr(), invstd0=inv_d.data_ptr(), scale0=sc_d.data_ptr(), shift0=sh_d.data_ptr(),
                     partials=parts.data_ptr() if with_partials else None, partials_bytes=pb if with_partials else 0)
        dx = torch.full((B, H, W, Cin), float("nan"), device=cuda)
        P = ctypes.c_int(-1)
        N.check(L.osi_conv_dgrad_fused_frozen(ctypes.byref(d), N.ptr(dy_d), N.ptr(w_d), N.ptr(dx), ctypes.byref(f), 0, ctypes.byref(P), T.S()),
                "osi_conv_dgrad_fused_frozen")
        torch.cuda.synchronize()
        if not with_partials:
            assert P.value == -1 and bool(torch.isnan(parts).all()), "partials = NULL: nothing but dx may be written"
            return dx, None, 0
        return dx, parts[:2 * P.value * Cin].clone().view(2, P.value, Cin), P.value

    if cus:
        N.check(L.osi_set_tuning(b"tail_cus", cus))
        N.check(L.osi_set_tuning(b"tail_mint", 2)); N.check(L.osi_set_tuning(b"tail_smax", 32))
    try:
        pb = L.osi_conv_dgrad_fused_workspace(ctypes.byref(d))
        N.check(L.osi_set_tuning(b"tail_split", 0))
        pb0 = L.osi_conv_dgrad_fused_workspace(ctypes.byref(d))
        g0, p0, P0 = run(pb0)                                                     # the un-split launch
        gn, _, _ = run(0, with_partials=False)                                    # the input-only form
        N.check(L.osi_set_tuning(b"tail_split", 1))
        if cus:
            assert pb > pb0, "this case is meant to have a split remainder"
        g1, p1, P1 = run(pb)
        g2, p2, _ = run(pb)
    finally:
        N.check(L.osi_set_tuning(b"tail_cus", 0))
        N.check(L.osi_set_tuning(b"tail_split", 1))
        N.check(L.osi_set_tuning(b"tail_mint", 16)); N.check(L.osi_set_tuning(b"tail_smax", 8))

    dgrad = torch.nn.grad.conv2d_input((B, Cin, H, W), T.oihw(w.double()), T.nchw(dy.double()), stride, pad).permute(0, 2, 3, 1).reshape(M, Cin)
    g_ref = dgrad * gate                                                          # g = gate . acc
    ref = g_ref * scale.double()                                                  # the store: dy0 = scale0 * g
    taps = k * k if stride == 1 else 4                                            # most taps that reach one input pixel
    tol = _bound(Cout * taps, ref)
    s = stride
    P_want = s * s * ((B * ((H + s - 1) // s) * ((W + s - 1) // s) + 63) // 64)
    assert P0 == P1 == P_want
    for name, got in (("unsplit", g0), ("partials = NULL", gn), ("default plan", g1)):
        got = got.cpu().view(M, Cin)
        assert bool(torch.isfinite(got).all()), f"{name}: an element of the NaN-poisoned output was not written"
        err = float((got.double() - ref).abs().max())
        print(f"frozen dgrad {kind} {(B, H, W, Cin, Cout, k, stride, cus)} {name}: max |err| {err:.3e} (bound {tol:.3e})")
        assert err <= tol, name
        assert bool((got[~gate] == 0).all()), f"{name}: a value behind a closed gate is not an exact zero"
    assert torch.equal(gn, g0), "the input-only form is the un-split launch without its sums: same bits"
    assert torch.equal(g1, g2) and torch.equal(p1, p2), "two calls differ"
    if cus:
        assert not torch.equal(g1, g0), "the split really changed the summation order of some tile"
    # the sums are over the UNSCALED g: merged in fp64 they are dbeta and dgamma of the producer's BatchNorm
    xhat = (y0.double() - mean.double()) * invstd.double()
    for name, parts in (("unsplit", p0), ("default plan", p1)):
        parts = parts.cpu().double().sum(1)
        for what, got, want in (("sum g", parts[0], g_ref.sum(0)), ("sum g xhat", parts[1], (g_ref * xhat).sum(0))):
            err = float((got - want).abs().max())
            print(f"    {name} {what}: max |err| {err:.3e} (bound {_bound(M, want):.3e})")
            assert err <= _bound(M, want), (name, what)


# ---- 4. frozen BatchNorm backward with a bitmask gate ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["positive", "signed"])
@pytest.mark.parametrize("C,two", [(64, False), (64, True), (256, False), (256, True)])
def test_frozen_bn_backward_bitmask_vs_fp64(cuda, C, two, kind):
    import osi_testlib as T
    L = N.lib()
    M = 297
    gen = torch.Generator().manual_seed(31 * C + two + (5 if kind == "signed" else 0))
    nc = 2 if two else 1
    bns = [_frozen_bn(C, gen, kind) for _ in range(nc)]
    ys = [torch.randn(M, C, generator=gen) * 2 + 0.5 for _ in range(nc)]
    dout = torch.randn(M, C, generator=gen)
    dev = lambda t: t.contiguous().to(cuda)
    ys_d = [dev(y) for y in ys]
    bn_d = [[dev(t) for t in b] for b in bns]                                    # gamma, beta, mean, invstd, scale, shift
    # the block output's bitmask as the forward writes it: relu(bn3(y0) [+ bn_d(y1)]) > 0
    act = torch.empty(M, C, device=cuda)
    mask = torch.zeros(L.osi_bn_relu_mask_bytes(M, C), dtype=torch.uint8, device=cuda)
    if two:
        N.check(L.osi_bn_apply_relu_mask2(N.ptr(ys_d[0]), N.ptr(bn_d[0][4]), N.ptr(bn_d[0][5]), N.ptr(ys_d[1]), N.ptr(bn_d[1][4]), N.ptr(bn_d[1][5]),
                                          N.ptr(act), N.ptr(mask), M, C, T.S()))
    else:
        N.check(L.osi_bn_apply_relu_mask(N.ptr(ys_d[0]), None, N.ptr(bn_d[0][4]), N.ptr(bn_d[0][5]), N.ptr(act), N.ptr(mask), M, C, T.S()))
    gate = (act > 0).cpu()
    if kind == "signed" and not two:
        assert float((0.05 * bns[0][3] * (ys[0] - bns[0][2]).abs().max(0).values).max()) < 1.0
        T.assert_signed_gates(gate, C, "block-output bitmask")
    wsb = L.osi_bn_backward_workspace(M, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)

    def run(reduce, inplace, use_mask=True, src=None):
        src = dev(dout) if src is None else src.clone()
        dys = [src if (inplace and i == 0) else torch.full((M, C), float("nan"), device=cuda) for i in range(nc)]
        dgs = [torch.full((C,), float("nan"), device=cuda) for _ in range(nc)]
        dbs = [torch.full((C,), float("nan"), device=cuda) for _ in range(nc)]
        gm = torch.full((M, C), float("nan"), device=cuda)
        cs = (N.BnFrozenConsumer * 2)()
        for i in range(nc):
            cs[i] = N.BnFrozenConsumer(ys_d[i].data_ptr(), bn_d[i][2].data_ptr(), bn_d[i][3].data_ptr(), bn_d[i][4].data_ptr(), dys[i].data_ptr(),
                                       dgs[i].data_ptr() if reduce else None, dbs[i].data_ptr() if reduce else None)
        N.check(L.osi_bn_backward_frozen(N.ptr(src), N.ptr(mask) if use_mask else None, cs, nc, N.ptr(gm), M, C, N.ptr(ws), wsb, T.S()),
                "osi_bn_backward_frozen")
        torch.cuda.synchronize()
        return dys, dgs, dbs, gm

    g_ref = dout.double() * gate
    dys, dgs, dbs, gm = run(True, False)
    dys2, dgs2, dbs2, gm2 = run(True, True)                                       # dy0 written over dout
    assert torch.equal(gm.cpu().double(), g_ref), "gmasked is the gated gradient itself"
    for i in range(nc):
        gamma, beta, mean, invstd, scale, shift = bns[i]
        ref = g_ref * scale.double()
        got = dys[i].cpu()
        assert bool(torch.isfinite(got).all())
        err = float((got.double() - ref).abs().max())
        print(f"frozen bn bwd {kind} C={C} consumers={nc} [{i}]: dy max |err| {err:.3e} (bound {_bound(1, ref):.3e})")
        assert err <= _bound(1, ref)
        assert bool((got[~gate] == 0).all())
        assert torch.equal(dys2[i], dys[i]) and torch.equal(dgs2[i], dgs[i]) and torch.equal(dbs2[i], dbs[i]), "in place / two calls differ"
        xhat = (ys[i].double() - mean.double()) * invstd.double()
        for what, g, want in (("dbeta", dbs[i], g_ref.sum(0)), ("dgamma", dgs[i], (g_ref * xhat).sum(0))):
            err = float((g.cpu().double() - want).abs().max())
            print(f"    {what}: max |err| {err:.3e} (bound {_bound(M, want):.3e})")
            assert err <= _bound(M, want), what
    # no parameter gradient asked for: no reduction runs (the poisoned vectors stay poisoned), the same dy bits
    dys3, dgs3, dbs3, _ = run(False, False)
    for i in range(nc):
        assert torch.equal(dys3[i], dys[i])
        assert bool(torch.isnan(dgs3[i]).all()) and bool(torch.isnan(dbs3[i]).all())
    # relu_mask = NULL: the gradient arrives gated (a dgrad epilogue did it): dy = scale * dout, nothing else
    dys4, _, _, gm4 = run(False, False, use_mask=False, src=gm)
    for i in range(nc):
        assert torch.equal(dys4[i], dys[i])
    assert torch.equal(gm4, gm)


# ---- 5. frozen stem tail -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["positive", "signed"])
@pytest.mark.parametrize("B,Hi,Wi", [(2, 32, 32), (2, 37, 45)])
def test_frozen_stem_tail_vs_fp64(cuda, B, Hi, Wi, kind):
    """Image size Hi x Wi -> stem output H x W = 16 x 16 / 19 x 23 (odd: the pooled border windows are cut). The max-pool scatter and the
    bit-7 gate are decoded from the arg-max bytes the forward kernel wrote (what the backward itself reads)."""
    import osi_testlib as T
    L = N.lib()
    C = 64
    H, W = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M = B * H * W
    gen = torch.Generator().manual_seed(Hi * 100 + Wi + (3 if kind == "signed" else 0))
    gamma, beta, mean, invstd, scale, shift = _frozen_bn(C, gen, kind)
    y = torch.randn(B, H, W, C, generator=gen) * 2 + 0.5
    gpool = torch.randn(B, Ho, Wo, C, generator=gen)
    dev = lambda t: t.contiguous().to(cuda)
    y_d, gp_d, mean_d, inv_d, sc_d, sh_d = map(dev, (y, gpool, mean, invstd, scale, shift))
    pooled = torch.empty(B, Ho, Wo, C, device=cuda)
    idx = torch.zeros(B, Ho, Wo, C, dtype=torch.uint8, device=cuda)
    N.check(L.osi_bn_relu_maxpool_fwd(N.ptr(y_d), N.ptr(sc_d), N.ptr(sh_d), N.ptr(pooled), N.ptr(idx), B, H, W, C, T.S()))
    torch.cuda.synchronize()
    byte = idx.cpu().long()
    gate, tap = (byte >> 7).bool(), byte & 0x7F
    if kind == "signed":
        assert float((0.05 * invstd * (y.reshape(M, C) - mean).abs().max(0).values).max()) < 1.0
        T.assert_signed_gates(gate, C, "bit 7 of the arg-max bytes")
    # G[b, h, w, c] = sum of the pooled gradients of the windows whose arg-max is (h, w) and whose maximum was positive
    ho = torch.arange(Ho).view(1, Ho, 1, 1)
    wo = torch.arange(Wo).view(1, 1, Wo, 1)
    hh, ww = ho * 2 - 1 + tap // 3, wo * 2 - 1 + tap % 3
    assert bool(((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W))[gate].all())
    b_i = torch.arange(B).view(B, 1, 1, 1).expand_as(tap)
    c_i = torch.arange(C).view(1, 1, 1, C).expand_as(tap)
    flat = ((b_i * H + hh) * W + ww) * C + c_i
    G = torch.zeros(M * C, dtype=torch.float64)
    G.index_add_(0, flat[gate], gpool.double()[gate])
    G = G.view(M, C)
    wsb = L.osi_bn_backward_workspace(M, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)

    def run(reduce):
        dy = torch.full((M, C), float("nan"), device=cuda)
        dg, db = torch.full((C,), float("nan"), device=cuda), torch.full((C,), float("nan"), device=cuda)
        N.check(L.osi_bn_relu_maxpool_bwd_frozen(N.ptr(gp_d), N.ptr(idx), N.ptr(y_d), N.ptr(mean_d), N.ptr(inv_d), N.ptr(sc_d), N.ptr(dy),
                                                 N.ptr(dg) if reduce else None, N.ptr(db) if reduce else None, B, H, W, C, N.ptr(ws), wsb, T.S()),
                "osi_bn_relu_maxpool_bwd_frozen")
        torch.cuda.synchronize()
        return dy, dg, db

    dy, dg, db = run(True)
    dy2, dg2, db2 = run(True)
    dy3, dg3, db3 = run(False)
    assert torch.equal(dy, dy2) and torch.equal(dg, dg2) and torch.equal(db, db2), "two calls differ"
    assert torch.equal(dy3, dy) and bool(torch.isnan(dg3).all()) and bool(torch.isnan(db3).all()), "no reduction without parameter gradients"
    ref = G * scale.double()
    got = dy.cpu()
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - ref).abs().max())
    print(f"frozen stem tail {kind} B={B} {Hi}x{Wi}: dy max |err| {err:.3e} (bound {_bound(4, ref):.3e})")
    assert err <= _bound(4, ref)                                                  # at most four windows meet in one pixel
    assert bool((got[G == 0] == 0).all())
    xhat = (y.double().view(M, C) - mean.double()) * invstd.double()
    for what, g, want in (("dbeta", db, G.sum(0)), ("dgamma", dg, (G * xhat).sum(0))):
        err = float((g.cpu().double() - want).abs().max())
        print(f"    {what}: max |err| {err:.3e} (bound {_bound(M, want):.3e})")
        assert err <= _bound(M, want), what


# ---- 6. the coefficient launch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["positive", "signed"])
def test_frozen_coefficients_one_launch_vs_fp64_and_eval_coeffs(cuda, kind):
    import osi_testlib as T
    L = N.lib()
    gen = torch.Generator().manual_seed(99 if kind == "signed" else 98)
    Cs = [64, 256, 2048, 100, 64]
    tab = (N.BnFrozenLayer * len(Cs))()
    keep = []
    for j, C in enumerate(Cs):
        gamma, beta = T.bn_state(C, gen, kind)
        rm, rv = 0.1 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
        src = [t.to(cuda) for t in (rm, rv, gamma, beta)]
        out = [torch.full((C,), float("nan"), device=cuda) for _ in range(4)]        # scale, shift, mean, invstd
        keep.append((src, out, (rm, rv, gamma, beta)))
        tab[j] = N.BnFrozenLayer(*[t.data_ptr() for t in src], *[t.data_ptr() for t in out], C)
    before = [[t.clone() for t in src] for src, _, _ in keep]
    N.check(L.osi_bn_frozen_coeffs_multi(tab, len(Cs), EPS, T.S()), "osi_bn_frozen_coeffs_multi")
    torch.cuda.synchronize()
    for (src, out, cpu), snap in zip(keep, before):
        rm, rv, gamma, beta = (t.double() for t in cpu)
        C = rm.numel()
        sc1, sh1 = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
        N.check(L.osi_bn_eval_coeffs(N.ptr(src[0]), N.ptr(src[1]), N.ptr(src[2]), N.ptr(src[3]), EPS, C, N.ptr(sc1), N.ptr(sh1), T.S()))
        torch.cuda.synchronize()
        assert torch.equal(out[0], sc1) and torch.equal(out[1], sh1), "scale / shift differ from osi_bn_eval_coeffs in some bit"
        assert torch.equal(out[2], src[0]), "mean is the running mean itself"
        inv = 1.0 / torch.sqrt(rv + EPS)
        for what, got, want in (("invstd", out[3], inv), ("scale", out[0], gamma * inv), ("shift", out[1], beta - rm * gamma * inv)):
            err = float((got.cpu().double() - want).abs().max())
            assert err <= _bound(1, want), (what, C, err)
        for a, b in zip(src, snap):
            assert torch.equal(a, b), "an input of the coefficient launch was written"


# ---- whole network -----------------------------------------------------------------------------------------------------------------
def _loss(logits, feats, wl, wf):
    return (logits * wl.to(logits.dtype)).sum() + (feats * wf.to(feats.dtype)).sum()


def _case(which):
    """(sd, x, wl, wf) on the CPU: the signed / zero_init_residual states at B = 4, 64 x 64 (osi_testlib.network_case), or
    B = 3 at 75 x 91 with C = 20 — a geometry without the fused stem tail, ragged tiles everywhere."""
    from oracle import resnet50_oracle as R
    import osi_testlib as T
    if which == "ragged":
        B, C = 3, 20
        gen = torch.Generator().manual_seed(7)
        sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), generator=gen)
        x = torch.rand(B, 3, 75, 91, generator=gen)
    else:
        sd, x, _ = T.network_case(which)
        B, C = T.NET_B, T.NET_C
    gen = torch.Generator().manual_seed(sum(map(ord, which)))
    return sd, x, torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen) * 0.1


def _model(sd, cuda):
    from openset_imagenet import ResNet50
    C = sd["logits.weight"].shape[0]
    model = ResNet50(C, C, False)
    model.load_state_dict(sd)
    return model.to(cuda)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _backward(model, x, wl, wf, want_x=True, route="backward"):
    """One forward + loss + backward of whatever route the model's state selects: (logits, features, x.grad or None, {name: grad})."""
    for p in model.parameters():
        p.grad = None
    xi = x.clone().requires_grad_(want_x)
    logits, feats = model(xi)
    loss = _loss(logits, feats, wl.to(x.device), wf.to(x.device))
    if route == "autograd":
        (gx,) = torch.autograd.grad(loss, xi)
    else:
        loss.backward()
        gx = xi.grad
    torch.cuda.synchronize()
    return logits.detach(), feats.detach(), (None if gx is None else gx.detach().clone()), _grads(model)


@functools.lru_cache(maxsize=None)
def _eval_run(which):
    """The eval-mode route of one case, run ONCE and shared (nothing below changes what it returns): model.eval(), x.requires_grad_()."""
    import osi_testlib as T
    cuda = torch.device("cuda:0")
    sd, x, wl, wf = _case(which)
    model = _model(sd, cuda).eval()
    buffers, nbt = model._flat_buffers.clone(), model._nbt.clone()
    xd = x.to(cuda)
    logits, feats, gx, grads = _backward(model, xd, wl, wf)
    gates = T.hip_gates(model)
    return dict(sd=sd, x=x, xd=xd, wl=wl, wf=wf, model=model, logits=logits, feats=feats, gx=gx, grads=grads, gates=gates,
                buffers=buffers, nbt=nbt)


def test_eval_mode_forward_is_differentiable_and_leaves_the_statistics_alone(cuda):
    """7. Fails on the parent: there an eval-mode forward returns tensors without a grad_fn. Outputs = the bits of the training topology
    on running statistics (executor option eval_fused = 0) under tail_split = 0; logits against the fp64 eval oracle."""
    from oracle import resnet50_oracle as R
    sd, x, wl, wf = _case("signed")
    L = N.lib()
    N.check(L.osi_set_tuning(b"tail_split", 0))           # a plan knob: before the executor exists
    try:
        model = _model(sd, cuda).eval()
        buffers, nbt = model._flat_buffers.clone(), model._nbt.clone()
        xd = x.to(cuda).requires_grad_()
        logits, feats = model(xd)
        assert logits.grad_fn is not None and feats.grad_fn is logits.grad_fn
        _loss(logits, feats, wl.to(cuda), wf.to(cuda)).backward()
        torch.cuda.synchronize()
        assert xd.grad is not None and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
        assert torch.equal(model._flat_buffers, buffers) and torch.equal(model._nbt, nbt)
        net = model._last[0]
        N.check(L.osi_resnet50_set_option(net.h, b"eval_fused", 0))
        with torch.no_grad():
            lg0, ft0 = model(xd.detach())
        torch.cuda.synchronize()
        assert torch.equal(logits.detach(), lg0) and torch.equal(feats.detach(), ft0)
        assert torch.equal(model._flat_buffers, buffers) and torch.equal(model._nbt, nbt)
        del model
    finally:
        N.check(L.osi_set_tuning(b"tail_split", 1))
    with torch.no_grad():
        ref, _ = R.forward({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}, x.double(), training=False)
    err = float((logits.detach().cpu().double() - ref).abs().max())
    print(f"eval-mode logits vs fp64 oracle: max |err| {err:.3e} at |logit| <= {float(ref.abs().max()):.2f}")
    assert err <= 1e-4 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("which", ["signed", "zero_init_residual", "ragged"])
def test_eval_mode_gradients_vs_fp64_oracle_under_the_hip_gates(cuda, which):
    """8. x.grad and all 162 gradients. Bar per tensor: 10 x the largest per-tensor error of the torch-CPU fp32 oracle in this same case
    (same gates), never above the project's 5e-4. Measured: see DESIGN section 4."""
    from test_frozen_bn_cpu import eval_oracle
    r = _eval_run(which)
    assert torch.equal(r["model"]._flat_buffers, r["buffers"]) and torch.equal(r["model"]._nbt, r["nbt"])
    _, gx64, g64, _ = eval_oracle(r["sd"], r["x"], r["wl"], r["wf"], torch.float64, gates=r["gates"])
    _, gx32, g32, _ = eval_oracle(r["sd"], r["x"], r["wl"], r["wf"], torch.float32, gates=r["gates"])
    assert len(r["grads"]) == 162 == len(g64)
    live = [k for k in g64 if float(g64[k].abs().max()) > 0]
    cpu_err = max([_rel(g32[k], g64[k]) for k in live] + [_rel(gx32, gx64)])
    bar = min(10 * cpu_err, GRAD_TOL)
    errs = {k: _rel(r["grads"][k].cpu(), g64[k]) for k in live}
    errs["x.grad"] = _rel(r["gx"].cpu(), gx64)
    worst = max(errs, key=errs.get)
    print(f"frozen gradients {which}: x.grad {errs['x.grad']:.2e}, worst tensor {errs[worst]:.2e} ({worst}), "
          f"median {sorted(errs.values())[len(errs) // 2]:.2e}; fp32 CPU oracle worst {cpu_err:.2e}, bar {bar:.2e}; "
          f"{len(g64) - len(live)} tensors exactly zero")
    for k in g64:
        if k not in live:        # e.g. gamma3 = 0 kills the whole main branch: exact zeros, not small numbers
            assert float(r["grads"][k].abs().max()) == 0.0, f"{k}: the reference is exactly zero"
    if which == "zero_init_residual":
        assert len(g64) - len(live) >= 16 * 7      # conv1 / bn1 / conv2 / bn2 / conv3 of every block
    for k, e in errs.items():
        assert e <= bar, f"{k}: rel-L2 {e:.2e} > {bar:.2e}"


def test_input_only_backward_same_bits_and_untouched_arena(cuda):
    """9."""
    r = _eval_run("signed")
    model = r["model"]
    try:
        for p in model.parameters():
            p.requires_grad_(False)
            p.grad = None
        model._flat_grads.fill_(float("nan"))
        _, _, gx, none = _backward(model, r["xd"], r["wl"], r["wf"])
        assert not none and torch.equal(gx, r["gx"]), "input-only x.grad differs from the full backward's"
        assert bool(torch.isnan(model._flat_grads).all()), "an input-only backward wrote the gradient arena"
        _, _, gx_ag, _ = _backward(model, r["xd"], r["wl"], r["wf"], route="autograd")
        assert torch.equal(gx_ag, r["gx"])
        assert bool(torch.isnan(model._flat_grads).all())
    finally:
        for p in model.parameters():
            p.requires_grad_(True)
        model._flat_grads.zero_()
    _, _, gx_ag, grads = _backward(model, r["xd"], r["wl"], r["wf"], route="autograd")     # torch.autograd.grad(loss, x) with live parameters
    assert torch.equal(gx_ag, r["gx"])


@pytest.mark.parametrize("layout", ["nchw", "nhwc4"])
def test_fgsm_in_eval_mode(cuda, layout):
    """10. next_backward(fgsm=eps) BEFORE the forward: it is what makes an eval-mode forward of a plain batch differentiable."""
    from openset_imagenet.adversary import fgsm_attack
    r = _eval_run("signed")
    model, xd, eps = r["model"], r["xd"], 0.03
    batch = xd
    if layout == "nhwc4":
        batch = torch.zeros(xd.shape[0], xd.shape[2], xd.shape[3], 4, device=cuda)
        batch[..., :3] = xd.permute(0, 2, 3, 1)
    model.next_backward(fgsm=eps)
    logits, feats = model(batch)
    assert logits.grad_fn is not None
    assert torch.equal(logits.detach(), r["logits"])
    _loss(logits, feats, r["wl"].to(cuda), r["wf"].to(cuda)).backward()
    torch.cuda.synchronize()
    adv = model.adversarial_batch()
    want = fgsm_attack(xd, r["gx"], eps).permute(0, 2, 3, 1)
    assert adv.shape == (xd.shape[0], xd.shape[2], xd.shape[3], 4)
    assert torch.equal(adv[..., :3], want)
    assert bool((adv[..., 3] == 0).all())
    assert torch.equal(model._flat_buffers, r["buffers"]) and torch.equal(model._nbt, r["nbt"])
    for k, g in _grads(model).items():
        assert torch.equal(g, r["grads"][k]), k


def test_freeze_bn_in_training_mode(cuda):
    """11."""
    from openset_imagenet import optim
    r = _eval_run("signed")
    sd, xd, wl, wf = r["sd"], r["xd"], r["wl"], r["wf"]
    model = _model(sd, cuda).train().freeze_bn()
    assert model.training and model.bn_frozen
    buffers, nbt = model._flat_buffers.clone(), model._nbt.clone()
    opt = optim.Adam(model.parameters(), lr=1e-3)
    params0 = model._flat_params.clone()
    lg, ft, gx, grads = _backward(model, xd, wl, wf)
    assert torch.equal(lg, r["logits"]) and torch.equal(gx, r["gx"]) and grads.keys() == r["grads"].keys()
    for k in grads:
        assert torch.equal(grads[k], r["grads"][k]), k
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(model._flat_params, params0), "the optimizer step moved nothing"
    assert torch.equal(model._flat_buffers, buffers) and torch.equal(model._nbt, nbt), "a frozen step touched the running statistics"
    with torch.no_grad():                                    # no graph, still frozen: the inference forward, statistics untouched
        model(xd)
    assert torch.equal(model._flat_buffers, buffers) and torch.equal(model._nbt, nbt)
    # released again: a training step is the one of a model that never froze
    model.load_state_dict(sd)
    assert model.freeze_bn(False) is model and not model.bn_frozen
    fresh = _model(sd, cuda).train()
    a = _backward(model, xd, wl, wf)
    b = _backward(fresh, xd, wl, wf)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    assert torch.equal(model._flat_buffers, fresh._flat_buffers) and torch.equal(model._nbt, fresh._nbt)
    assert not torch.equal(model._flat_buffers, buffers) and bool((model._nbt == nbt + 1).all())


class _NoComm:
    """stand-in for dp's gradient sync at world size 1: the model takes its stage-by-stage path"""

    def __init__(self):
        self.buckets = 0

    def bucket_ready(self, flat, lo, hi, handoff=None):
        self.buckets += 1

    def finish(self):
        pass


def test_staged_frozen_backward_same_bits(cuda):
    """12. stage_lo..stage_hi one at a time (the data-parallel order), with and without parameter gradients."""
    r = _eval_run("signed")
    model = r["model"]
    model._grad_sync = sync = _NoComm()
    try:
        _, _, gx, grads = _backward(model, r["xd"], r["wl"], r["wf"])
        assert sync.buckets == model._n_stages
        for p in model.parameters():
            p.requires_grad_(False)
        _, _, gx_only, _ = _backward(model, r["xd"], r["wl"], r["wf"])
        assert sync.buckets == model._n_stages
    finally:
        model._grad_sync = None
        for p in model.parameters():
            p.requires_grad_(True)
    assert torch.equal(gx, r["gx"]) and torch.equal(gx_only, r["gx"])
    for k in grads:
        assert torch.equal(grads[k], r["grads"][k]), k


def test_state_errors(cuda):
    """13."""
    r = _eval_run("signed")
    model, xd = r["model"], r["xd"]
    L = N.lib()
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    logits, feats = model(xd.clone().requires_grad_())          # frozen forward ...
    net = model._last[0]
    with torch.no_grad():
        model(xd)                                                # ... replaced by an inference forward: nothing left to differentiate
    dl = torch.zeros_like(logits)
    dimg = torch.empty_like(xd)
    assert L.osi_resnet50_backward(net.h, N.ptr(model._flat_params), N.ptr(model._flat_grads), N.ptr(model._ws), N.ptr(dl), None, 0, 1, st()) == -3
    assert L.osi_resnet50_backward_ex(net.h, N.ptr(model._flat_params), None, N.ptr(model._ws), N.ptr(dl), None, N.ptr(dimg), 0, 0, 4, st()) == -3
    with pytest.raises(RuntimeError, match="no longer the model's latest"):
        _loss(logits, feats, r["wl"].to(cuda), r["wf"].to(cuda)).backward()
    # a later stage of a frozen backward that changes the request is refused; the backward can still be finished
    logits, feats = model(xd.clone().requires_grad_())
    wl_d, wf_d = r["wl"].to(cuda).contiguous(), r["wf"].to(cuda).contiguous()
    args = lambda dimage, s: (net.h, N.ptr(model._flat_params), N.ptr(model._flat_grads), N.ptr(model._ws), N.ptr(wl_d), N.ptr(wf_d),
                              N.ptr(dimage), 1, s, s + 1, st())
    assert L.osi_resnet50_backward_ex(*args(dimg, 0)) == 0
    assert L.osi_resnet50_backward_ex(*args(None, 1)) == -3
    for s in range(1, model._n_stages):
        assert L.osi_resnet50_backward_ex(*args(dimg, s)) == 0
    torch.cuda.synchronize()
    assert torch.equal(dimg, r["gx"])
    # next_backward(fgsm=...) after an eval-mode inference forward (grad enabled, plain batch): too late, and said so
    lg, _ = model(xd)
    assert lg.grad_fn is None
    with pytest.raises(RuntimeError, match="BEFORE the forward"):
        model.next_backward(fgsm=0.01)
    assert model._bw_request is None
    with torch.no_grad():                                        # validate()'s forwards do not get in the way of a later request
        model(xd)
    model.next_backward(fgsm=0.01)
    model._bw_request = None

"""GPU: projected attacks (ABI 19). Like the FGSM path before it, the new path is a composition of pieces that are held to fp64
elsewhere, so almost every check here is torch.equal:
  1. osi_stem_dgrad_pgd against pgd_step of what osi_stem_dgrad writes, the two FGSM identities, its signs against fp64, argument rules;
  2. osi_resnet50_backward_attack: input-only against backward_ex(dimage, 0) + pgd_step, full against backward_adv, staged, state and
     aliasing rules, the three input forms — after the training forward and after the frozen-statistics forward;
  3. ResNet50.next_backward(pgd=..., input_only=True), adversary.pgd_attack, train() with who: pgd and validate() with adv.validate
     against loops written out of public pieces."""
import ctypes
import functools
import math

import pytest
import torch

from openset_imagenet import _native as N
from openset_imagenet import adversary as A

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
EPS, ALPHA = 8.0 / 255.0, 2.0 / 255.0
INF = float("inf")
STEPS_AE = ((ALPHA, EPS), (EPS, EPS), (-ALPHA, EPS), (ALPHA, 0.0), (ALPHA, INF))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc4(x, lane3=0.0):
    """NCHW [B, 3, H, W] -> NHWC4 [B, H, W, 4] with the 4th lane set to `lane3`"""
    B, _, H, W = x.shape
    out = torch.full((B, H, W, 4), float(lane3), device=x.device, dtype=x.dtype)
    out[..., :3] = x.permute(0, 2, 3, 1)
    return out


def _nan_like(t):
    return torch.full_like(t, float("nan"))


# ---- 1. kernel -------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 32, 32), (1, 33, 65), (3, 70, 130), (2, 96, 128)]     # one partial tile; odd and ragged over several 32 x 64 tiles; whole tiles


@functools.lru_cache(maxsize=None)
def _kernel_case(B, H, W):
    """inputs as test_stem_dgrad_fgsm_kernel draws them, plus an iterate inside the eps-ball of the anchor; osi_stem_dgrad's own dx and
    the fp64 gradient, computed once per shape"""
    cuda = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(B * 1000 + H + W)
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = torch.randn(64, 3, 7, 7, generator=gen) * 0.1
    dy = torch.randn(B, 64, Hs, Ws, generator=gen)
    anchor = torch.rand(B, 3, H, W, generator=gen)
    x_cur = (anchor + EPS * (2.0 * torch.rand(B, 3, H, W, generator=gen) - 1.0)).clamp(0.0, 1.0)
    w_krsc3 = w.permute(0, 2, 3, 1).contiguous().to(cuda)
    dy_nhwc = dy.permute(0, 2, 3, 1).contiguous().to(cuda)
    dx = torch.full((B, 3, H, W), float("nan"), device=cuda)
    N.check(N.lib().osi_stem_dgrad(N.ptr(dy_nhwc), N.ptr(w_krsc3), N.ptr(dx), B, H, W, _stream()), "osi_stem_dgrad")
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_input((B, 3, H, W), w.double(), dy.double(), stride=2, padding=3)
    return dict(w=w_krsc3, dy=dy_nhwc, anchor=anchor, x_cur=x_cur, dx=dx, ref=ref)


def _pgd(case, x4, a4, out, alpha, eps, lo=0.0, hi=1.0):
    B, H, W, _ = out.shape
    return N.lib().osi_stem_dgrad_pgd(N.ptr(case["dy"]), N.ptr(case["w"]), N.ptr(x4), N.ptr(a4), N.ptr(out), alpha, eps, lo, hi, B, H, W, _stream())


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_stem_dgrad_pgd_kernel(cuda, B, H, W):
    """Bit-equal to pgd_step of osi_stem_dgrad's own dx for every (alpha, eps); two calls equal; every element written, lane 3 zero;
    against fp64 the pixel is the fp64 gradient's choice everywhere except where |dx_fp64| is below the kernel's own error bound (the
    FGSM test's twin and excluded set), and that excluded share stays <= 1e-4."""
    case = _kernel_case(B, H, W)
    xc, xa, dx, ref = case["x_cur"].to(cuda), case["anchor"].to(cuda), case["dx"], case["ref"]
    x4, a4 = _nhwc4(xc, lane3=0.5), _nhwc4(xa, lane3=-0.25)      # whatever the inputs hold in their 4th lane, x_next's is zero
    thr = (2e-6 + 6e-8 * math.sqrt(64 * 49)) * float(ref.abs().max())
    excluded = ref.abs() <= thr
    share = float(excluded.double().mean())
    sign64 = torch.sign(ref).float()
    for alpha, eps in STEPS_AE:
        outs = []
        for _ in range(2):
            out = torch.full((B, H, W, 4), float("nan"), device=cuda)
            N.check(_pgd(case, x4, a4, out, alpha, eps), "osi_stem_dgrad_pgd")
            torch.cuda.synchronize()
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), "two calls differ"
        got = outs[0]
        assert torch.isfinite(got).all(), "an element of x_next was not written"
        want = _nhwc4(A.pgd_step(xc, dx, xa, alpha, eps))
        assert torch.equal(got, want), f"alpha={alpha} eps={eps}: x_next is not pgd_step(x_cur, osi_stem_dgrad's dx, anchor)"
        assert bool((got[..., 3] == 0).all())
        if eps == 0.0:
            assert torch.equal(got[..., :3], a4[..., :3])
        twin = A.pgd_step(case["x_cur"], sign64, case["anchor"], alpha, eps)
        diff = got[..., :3].permute(0, 3, 1, 2).cpu() != twin
        outside = int((diff & ~excluded).sum())
        print(f"stem dgrad pgd B={B} {H}x{W} alpha={alpha:.4f} eps={eps:.4f}: excluded share {share:.2e} (|dx64| <= {thr:.3e}), "
              f"{int(diff.sum())} pixels differ from the fp64 twin, {outside} of them outside the excluded set")
        assert outside == 0
    assert share <= 1e-4


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_stem_dgrad_pgd_fgsm_identities(cuda, B, H, W):
    """anchor == iterate and 0 <= alpha <= eps, or eps = +inf with any anchor: the bits of osi_stem_dgrad_fgsm(eps := alpha)"""
    case = _kernel_case(B, H, W)
    x4, a4 = _nhwc4(case["x_cur"].to(cuda), lane3=0.5), _nhwc4(case["anchor"].to(cuda), lane3=-0.25)
    lib = N.lib()

    def fgsm(step):
        out = torch.full((B, H, W, 4), float("nan"), device=cuda)
        N.check(lib.osi_stem_dgrad_fgsm(N.ptr(case["dy"]), N.ptr(case["w"]), N.ptr(x4), N.ptr(out), step, 0.0, 1.0, B, H, W, _stream()),
                "osi_stem_dgrad_fgsm")
        return out

    for alpha, eps, anchor in ((ALPHA, EPS, x4), (EPS, EPS, x4), (0.0, EPS, x4), (ALPHA, INF, a4), (EPS, INF, a4), (ALPHA, INF, x4)):
        out = torch.full((B, H, W, 4), float("nan"), device=cuda)
        N.check(_pgd(case, x4, anchor, out, alpha, eps), "osi_stem_dgrad_pgd")
        torch.cuda.synchronize()
        assert torch.equal(out, fgsm(alpha)), (alpha, eps, anchor is x4)


def test_stem_dgrad_pgd_argument_rules_leave_the_output_alone(cuda):
    B, H, W = SHAPES[0]
    case = _kernel_case(B, H, W)
    x4, a4 = _nhwc4(case["x_cur"].to(cuda)), _nhwc4(case["anchor"].to(cuda))
    out = torch.full((B, H, W, 4), float("nan"), device=cuda)
    f = N.lib().osi_stem_dgrad_pgd
    dy, w, x, a, o = N.ptr(case["dy"]), N.ptr(case["w"]), N.ptr(x4), N.ptr(a4), N.ptr(out)
    st = _stream()
    assert f(dy, w, x, None, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG            # the anchor is not optional here
    assert f(dy, w, x, a + 4, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG           # ... and is loaded as 16-byte vectors
    assert f(dy, w, x + 8, a, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG
    assert f(dy, w, x, a, o + 4, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG
    assert f(dy, w, x, a, o, INF, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG                 # alpha finite
    assert f(dy, w, x, a, o, -INF, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG
    assert f(dy, w, x, a, o, float("nan"), EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG
    assert f(dy, w, x, a, o, ALPHA, -1e-3, 0.0, 1.0, B, H, W, st) == ERR_ARG             # eps >= 0
    assert f(dy, w, x, a, o, ALPHA, float("nan"), 0.0, 1.0, B, H, W, st) == ERR_ARG
    assert f(dy, w, x, a, o, ALPHA, EPS, 1.0, 0.0, B, H, W, st) == ERR_ARG               # lo <= hi
    assert f(dy, w, x, a, o, ALPHA, EPS, 0.0, 1.0, B, 31, W, st) == ERR_ARG
    assert f(dy, w, o, a, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG               # x_next is the iterate
    assert f(dy, w, x, o, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG               # x_next is the anchor
    assert f(dy, w, o + 64, a, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG          # ... or overlaps one of them
    assert f(dy, w, x, o - 64, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote x_next"
    assert f(dy, w, x, x, o, ALPHA, EPS, 0.0, 1.0, B, H, W, st) == 0                     # the anchor may be the iterate
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_torch_op_stem_dgrad_pgd(cuda):
    B, H, W = SHAPES[1]
    case = _kernel_case(B, H, W)
    x4, a4 = _nhwc4(case["x_cur"].to(cuda)), _nhwc4(case["anchor"].to(cuda))
    out = torch.full((B, H, W, 4), float("nan"), device=cuda)
    N.ops().stem_dgrad_pgd(case["dy"], case["w"], x4, a4, out, ALPHA, EPS, 0.0, 1.0)
    want = torch.full((B, H, W, 4), float("nan"), device=cuda)
    N.check(_pgd(case, x4, a4, want, ALPHA, EPS), "osi_stem_dgrad_pgd")
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    with pytest.raises(RuntimeError, match="shape"):
        N.ops().stem_dgrad_pgd(case["dy"], case["w"], x4, a4[:, :32], out, ALPHA, EPS, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="dy"):
        N.ops().stem_dgrad_pgd(case["dy"][:, :8].contiguous(), case["w"], x4, a4, out, ALPHA, EPS, 0.0, 1.0)


# ---- helpers for the whole-network tests (those of tests/test_adversarial_gpu.py) ------------------------------------------------
def _model(cuda, C, seed):
    from openset_imagenet import ResNet50
    from oracle import resnet50_oracle as R
    gen = torch.Generator().manual_seed(seed)
    sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), generator=gen)
    model = ResNet50(C, C, False)
    model.load_state_dict(sd)
    return model.to(cuda).train(), sd


def _snap(model):
    return model._flat_buffers.clone(), model._nbt.clone()


def _restore(model, snap):
    with torch.no_grad():
        model._flat_buffers.copy_(snap[0])
        model._nbt.copy_(snap[1])


def _entropic_dlogits(logits, y, C):
    """dJ/dlogits of the entropic loss, through the loss kernel on detached logits (no route into the network)"""
    from openset_imagenet import EntropicOpensetLoss
    lg = logits.detach().clone().requires_grad_()
    EntropicOpensetLoss(C, 1.0)(lg, y).backward()
    return lg.grad.contiguous()


def _same_grads(model, a, b):
    assert len(model._pinfo) == 162
    for (name, off, numel, _) in model._pinfo:
        assert torch.isfinite(a[off:off + numel]).all(), f"{name}: not written"
        assert torch.equal(a[off:off + numel], b[off:off + numel]), name


def _frozen_copy(cuda, sd, C):
    """a second model of the same weights with every parameter frozen: its backward is input-only and leaves x.grad (the public
    route to dJ/dx that writes no parameter gradient)"""
    from openset_imagenet import ResNet50
    ref = ResNet50(C, C, False)
    ref.load_state_dict(sd)
    ref = ref.to(cuda)
    for p in ref.parameters():
        p.requires_grad_(False)
    return ref


# ---- 2. executor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["training", "frozen"])
def test_backward_attack_against_backward_ex_backward_adv_and_pgd_step(cuda, mode):
    B, HW, C = 8, 64, 10
    model, _ = _model(cuda, C, 41)
    model.freeze_bn(mode == "frozen")
    lib = N.lib()
    gen = torch.Generator().manual_seed(43)
    u8 = torch.randint(0, 256, (B, HW, HW, 3), generator=gen, dtype=torch.uint8)
    x = u8.permute(0, 3, 1, 2).float().div(255).contiguous().to(cuda)     # the NCHW batch u8 / 255 (true division, on the host)
    anchor = (x + EPS * (2.0 * torch.rand(B, 3, HW, HW, generator=gen).to(cuda) - 1.0)).clamp(0.0, 1.0)   # the forward's batch is the iterate
    a4 = _nhwc4(anchor)
    y = torch.randint(-1, C, (B,), generator=gen).to(cuda)
    snap = _snap(model)
    S = model._n_stages
    P = model._flat_params

    def forward(image):
        _restore(model, snap)
        logits, _ = model(image)
        return model._last[0], _entropic_dlogits(logits, y, C)

    def attack(net, dl, req, g, pg, s0=0, s1=S):
        return lib.osi_resnet50_backward_attack(net.h, N.ptr(P), None if g is None else N.ptr(g), N.ptr(model._ws), N.ptr(dl), None,
                                                ctypes.byref(req), pg, s0, s1, _stream())

    def request(xn, anchor4=a4, alpha=ALPHA, eps=EPS, lo=0.0, hi=1.0):
        return N.Attack(N.ptr(xn), None if anchor4 is None else N.ptr(anchor4), alpha, eps, lo, hi)

    # ---- input-only: backward_ex(dimage, param_grads = 0) is the yardstick
    net, dl = forward(x)
    dimage0 = torch.empty(B, 3, HW, HW, device=cuda)
    assert lib.osi_resnet50_backward_ex(net.h, N.ptr(P), None, N.ptr(model._ws), N.ptr(dl), None, N.ptr(dimage0), 0, 0, S, _stream()) == 0
    torch.cuda.synchronize()
    for alpha, eps, anc in ((ALPHA, EPS, a4), (-ALPHA, EPS, a4), (ALPHA, INF, a4), (ALPHA, EPS, None), (EPS, EPS, None)):
        net2, dl2 = forward(x)
        assert net2 is net and torch.equal(dl2, dl)
        arena = _nan_like(model._flat_grads)
        xn = torch.full((B, HW, HW, 4), float("nan"), device=cuda)
        assert attack(net, dl, request(xn, anc, alpha, eps), arena if anc is not None else None, 0) == 0
        torch.cuda.synchronize()
        want = _nhwc4(A.pgd_step(x, dimage0, anchor if anc is not None else x, alpha, eps))
        assert torch.equal(xn, want), f"alpha={alpha} eps={eps}: x_next is not pgd_step of backward_ex(dimage, 0)'s dimage"
        assert bool(torch.isnan(arena).all()), "an input-only backward wrote into the gradient arena"
    want0 = _nhwc4(A.pgd_step(x, dimage0, anchor, ALPHA, EPS))

    # ---- parameter gradients: {x_adv, NULL, eps, eps} is backward_adv, bit for bit
    forward(x)
    g_adv = _nan_like(model._flat_grads)
    xa = torch.full((B, HW, HW, 4), float("nan"), device=cuda)
    assert lib.osi_resnet50_backward_adv(net.h, N.ptr(P), N.ptr(g_adv), N.ptr(model._ws), N.ptr(dl), None, N.ptr(xa), EPS, 0.0, 1.0, 0, S,
                                         _stream()) == 0
    forward(x)
    g_att = _nan_like(g_adv)
    xn = _nan_like(xa)
    assert attack(net, dl, request(xn, None, EPS, EPS), g_att, 1) == 0
    torch.cuda.synchronize()
    _same_grads(model, g_att, g_adv)
    assert torch.equal(xn, xa)
    # ... and an anchored step leaves the same parameter gradients and pgd_step of backward_ex(dimage, 1)'s dimage
    forward(x)
    g_ex = _nan_like(g_adv)
    dimage1 = torch.empty_like(dimage0)
    assert lib.osi_resnet50_backward_ex(net.h, N.ptr(P), N.ptr(g_ex), N.ptr(model._ws), N.ptr(dl), None, N.ptr(dimage1), 1, 0, S, _stream()) == 0
    forward(x)
    g_pgd = _nan_like(g_adv)
    xn = _nan_like(xa)
    assert attack(net, dl, request(xn), g_pgd, 1) == 0
    torch.cuda.synchronize()
    _same_grads(model, g_pgd, g_ex)
    _same_grads(model, g_adv, g_ex)
    assert torch.equal(xn, _nhwc4(A.pgd_step(x, dimage1, anchor, ALPHA, EPS)))

    # ---- stage by stage; a later stage with another request is refused and the backward can still be finished
    for pg in (0, 1):
        forward(x)
        g_st = _nan_like(g_adv)
        xn_st = _nan_like(xa)
        other = torch.empty_like(xa)
        assert attack(net, dl, request(xn_st), g_st, pg, 0, 1) == 0
        assert attack(net, dl, request(other), g_st, pg, 1, 2) == ERR_STATE
        assert attack(net, dl, request(xn_st, other), g_st, pg, 1, 2) == ERR_STATE
        assert attack(net, dl, request(xn_st, None), g_st, pg, 1, 2) == ERR_STATE
        assert attack(net, dl, request(xn_st, alpha=EPS), g_st, pg, 1, 2) == ERR_STATE
        assert attack(net, dl, request(xn_st, eps=EPS / 2), g_st, pg, 1, 2) == ERR_STATE
        assert attack(net, dl, request(xn_st, lo=-1.0), g_st, pg, 1, 2) == ERR_STATE
        assert attack(net, dl, request(xn_st, hi=2.0), g_st, pg, 1, 2) == ERR_STATE
        assert attack(net, dl, request(xn_st), g_st, 1 - pg, 1, 2) == ERR_STATE
        assert lib.osi_resnet50_backward_adv(net.h, N.ptr(P), N.ptr(g_st), N.ptr(model._ws), N.ptr(dl), None, N.ptr(xn_st), EPS, 0.0, 1.0, 1, 2,
                                             _stream()) == ERR_STATE
        for s in range(1, S):
            assert attack(net, dl, request(xn_st), g_st, pg, s, s + 1) == 0
        torch.cuda.synchronize()
        if pg:
            _same_grads(model, g_st, g_ex)
            assert torch.equal(xn_st, _nhwc4(A.pgd_step(x, dimage1, anchor, ALPHA, EPS)))
        else:
            assert bool(torch.isnan(g_st).all())
            assert torch.equal(xn_st, want0)
        assert attack(net, dl, request(xn_st), g_st, pg) == ERR_STATE          # the backward is over

    # ---- the equal NHWC4 batch bound in place: the aliasing rules, then the same bits; then the staged uint8 batch
    x4 = _nhwc4(x)
    net4, dl4 = forward(x4)
    assert net4 is net and torch.equal(dl4, dl)
    xn4 = _nan_like(xa)
    assert attack(net, dl, request(x4), None, 0) == ERR_ARG                                        # x_next = the bound input
    assert attack(net, dl, request(model._ws.view(torch.float32)[1024:]), None, 0) == ERR_ARG      # inside the workspace
    assert attack(net, dl, request(xn4, xn4), None, 0) == ERR_ARG                                  # x_next = the anchor
    assert attack(net, dl, request(xn4), None, 1) == ERR_ARG                                       # parameter gradients without an arena
    assert attack(net, dl, request(xn4), None, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(xn4, want0)
    assert torch.equal(x4, _nhwc4(x)) and torch.equal(a4, _nhwc4(anchor)), "an input batch was written"
    net8, dl8 = forward(u8.to(cuda))
    assert net8 is net and torch.equal(dl8, dl)
    xn8 = _nan_like(xa)
    assert attack(net, dl, request(xn8), None, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(xn8, want0)


def test_backward_attack_refused_behind_an_inference_form_prefix(cuda):
    B, HW, C = 8, 64, 10
    model, _ = _model(cuda, C, 45)
    model.freeze_below("layer2")
    x = torch.rand(B, 3, HW, HW, device=cuda)
    logits, _ = model(x)                                   # the prefix ran in the inference form: no image gradient behind it
    net = model._last[0]
    dl = torch.ones_like(logits)
    xn = torch.full((B, HW, HW, 4), float("nan"), device=cuda)
    req = N.Attack(N.ptr(xn), None, ALPHA, EPS, 0.0, 1.0)
    for pg in (0, 1):
        assert N.lib().osi_resnet50_backward_attack(net.h, N.ptr(model._flat_params), N.ptr(model._flat_grads), N.ptr(model._ws), N.ptr(dl), None,
                                                    ctypes.byref(req), pg, 0, model._n_stages, _stream()) == ERR_STATE
    torch.cuda.synchronize()
    assert bool(torch.isnan(xn).all())
    with pytest.raises(RuntimeError, match="x_next"):
        N.ops().resnet50_backward_attack(net.h.value, model._flat_params, model._flat_grads, model._ws, dl, None, xn[:, :32].contiguous(), None,
                                         ALPHA, EPS, 0.0, 1.0, True, 0, model._n_stages)
    with pytest.raises(RuntimeError, match="x_anchor"):
        N.ops().resnet50_backward_attack(net.h.value, model._flat_params, model._flat_grads, model._ws, dl, None, xn, xn[:4].contiguous(),
                                         ALPHA, EPS, 0.0, 1.0, True, 0, model._n_stages)


# ---- 3. model and loop -----------------------------------------------------------------------------------------------------------------
def _hand_attack(ref, x, y, loss, steps, start=None):
    """`steps` projected steps out of public pieces: an image that requires grad on the frozen-statistics route of a model whose
    parameters are all frozen (input-only backward), x.grad, pgd_step"""
    ref.eval()
    xk = x if start is None else start
    for _ in range(steps):
        xi = xk.clone().requires_grad_()
        loss(ref(xi)[0], y).backward()
        xk = A.pgd_step(xi.detach(), xi.grad, x, ALPHA, EPS)
    return xk


@pytest.mark.parametrize("training", [True, False])
def test_pgd_attack_equals_three_hand_composed_steps(cuda, training):
    from openset_imagenet import EntropicOpensetLoss
    B, HW, C = 8, 64, 10
    model, sd = _model(cuda, C, 91)
    model.train(training)
    ref = _frozen_copy(cuda, sd, C)
    gen = torch.Generator().manual_seed(93)
    x = torch.rand(B, 3, HW, HW, generator=gen).to(cuda)
    y = torch.randint(-1, C, (B,), generator=gen).to(cuda)
    loss = EntropicOpensetLoss(C, 1.0)
    loss3 = lambda lg, ft, t: loss(lg, t)
    want = _nhwc4(_hand_attack(ref, x, y, loss, 3))
    # the model carries the gradients of an earlier step: the attack must leave them, and everything else, alone
    with torch.no_grad():
        model._flat_grads.copy_(torch.randn(model._flat_grads.shape, generator=gen).to(cuda))
    for fresh in (False, True):
        model._grads_fresh = fresh
        grads, bufs, nbt = model._flat_grads.clone(), model._flat_buffers.clone(), model._nbt.clone()
        for images in (x, _nhwc4(x)):
            got = A.pgd_attack(model, images, y, loss3, EPS, ALPHA, 3)
            torch.cuda.synchronize()
            assert got.shape == (B, HW, HW, 4) and got.data_ptr() == model.adversarial_batch().data_ptr()
            assert torch.equal(got, want)
        assert model.training is training and not model.bn_frozen and model._grads_fresh is fresh and model._bw_request is None
        assert torch.equal(model._flat_grads, grads) and torch.equal(model._flat_buffers, bufs) and torch.equal(model._nbt, nbt)
    assert torch.equal(A.pgd_attack(model, x, y, loss3, EPS, ALPHA, 1), _nhwc4(A.pgd_step(x, _hand_grad(ref, x, y, loss), x, ALPHA, EPS)))
    # random start: the noise drawn as one [B, 3, H, W] tensor from the generator
    r1 = A.pgd_attack(model, x, y, loss3, EPS, ALPHA, 2, random_start=True, generator=torch.Generator(device=cuda).manual_seed(7)).clone()
    r2 = A.pgd_attack(model, _nhwc4(x), y, loss3, EPS, ALPHA, 2, random_start=True, generator=torch.Generator(device=cuda).manual_seed(7))
    noise = torch.rand(x.shape, generator=torch.Generator(device=cuda).manual_seed(7), device=cuda)
    start = (x + EPS * (2.0 * noise - 1.0)).clamp(0.0, 1.0)
    assert torch.equal(r1, r2) and torch.equal(r1, _nhwc4(_hand_attack_from(ref, x, start, y, loss, 2)))
    lo_b, hi_b = torch.clamp(x - EPS, min=0.0), torch.clamp(x + EPS, max=1.0)
    r = r1[..., :3].permute(0, 3, 1, 2)
    assert bool((r >= lo_b).all()) and bool((r <= hi_b).all())
    assert model.training is training


def _hand_grad(ref, x, y, loss):
    ref.eval()
    xi = x.clone().requires_grad_()
    loss(ref(xi)[0], y).backward()
    return xi.grad


def _hand_attack_from(ref, x, start, y, loss, steps):
    return _hand_attack(ref, x, y, loss, steps, start)


def test_next_backward_request_rules(cuda):
    from openset_imagenet import EntropicOpensetLoss
    B, HW, C = 8, 64, 10
    model, _ = _model(cuda, C, 95)
    x = torch.rand(B, 3, HW, HW, device=cuda)
    y = torch.randint(-1, C, (B,)).to(cuda)
    loss = EntropicOpensetLoss(C, 1.0)
    for bad in (dict(input_only=True), dict(fgsm=EPS, input_only=True, accumulate=True), dict(fgsm=EPS, pgd=(ALPHA, EPS, None)),
                dict(pgd=(INF, EPS, None)), dict(pgd=(ALPHA, -EPS, None)), dict(pgd=(ALPHA, EPS, x)), dict(pgd=(ALPHA, EPS, _nhwc4(x).cpu()))):
        with pytest.raises(ValueError):
            model.next_backward(**bad)
        assert model._bw_request is None
    # an input-only request has to precede its forward, in every mode
    for mode in (model.train, model.eval):
        mode()
        j = loss(model(x.clone().requires_grad_(not model.training))[0], y)
        model.next_backward(pgd=(ALPHA, EPS, None), input_only=True)
        with pytest.raises(RuntimeError, match="PRECEDE"):
            j.backward()
        assert model._bw_request is None
    # a geometry mismatch of the anchor is the op's error; the request is consumed either way
    model.train()
    model.next_backward(pgd=(ALPHA, EPS, _nhwc4(x)[:4].contiguous()), input_only=True)
    j = loss(model(x)[0], y)
    with pytest.raises(RuntimeError, match="x_anchor"):
        j.backward()
    assert model._bw_request is None
    # fgsm with input_only: the FGSM batch without a parameter gradient; the buffer pair alternates when the batch is fed back
    model.eval()
    model._grads_fresh = False
    model.next_backward(fgsm=EPS, input_only=True)
    loss(model(x)[0], y).backward()
    first = model.adversarial_batch()
    model.next_backward(pgd=(ALPHA, EPS, _nhwc4(x)), input_only=True)
    loss(model(first)[0], y).backward()
    second = model.adversarial_batch()
    model.next_backward(pgd=(ALPHA, EPS, _nhwc4(x)), input_only=True)
    loss(model(second)[0], y).backward()
    third = model.adversarial_batch()
    assert first.data_ptr() != second.data_ptr() and third.data_ptr() == first.data_ptr()
    assert not model._grads_fresh
    torch.cuda.synchronize()


class Loader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = range(sum(int(y.shape[0]) for _, y in batches))


def _meter(m):
    return [m.val, m.avg, m.sum, m.count]


def _train_run(cuda, adv, batches, C, seed=67):
    from openset_imagenet import EntropicOpensetLoss, losses as L, optim, tools
    from openset_imagenet.train import train
    from openset_imagenet.util import NameSpace
    tools.set_device_gpu(0)
    model, sd = _model(cuda, C, seed)
    cfg = NameSpace({"parallel": True, "batch_size": batches[0][1].shape[0], "loss": {"type": "entropic"}, "adv": adv})
    trackers = {"j": L.AverageMeter(), "j_adv": L.AverageMeter()}
    train(model, Loader(batches), optim.Adam(model, lr=1e-3), EntropicOpensetLoss(C, 1.0), trackers, cfg)
    torch.cuda.synchronize()
    return model, sd, trackers


def _train_batches(cuda, C, steps, B=8, HW=64):
    gen = torch.Generator().manual_seed(61)
    return [(torch.rand(B, 3, HW, HW, generator=gen).to(cuda), torch.randint(-1, C, (B,), generator=gen).to(cuda)) for _ in range(steps)]


@pytest.mark.parametrize("layout", ["nchw", "nhwc4"])
def test_train_with_pgd_equals_the_hand_loop(cuda, layout):
    """train() with who: pgd, steps: 3 against a loop written out of public pieces (in the manner of test_adversarial_gpu._loop_case)"""
    from openset_imagenet import EntropicOpensetLoss, ResNet50, losses as L, optim
    C, STEPS, K = 10, 3, 3
    batches = _train_batches(cuda, C, STEPS)
    fed = [(_nhwc4(x), y) for x, y in batches] if layout == "nhwc4" else batches
    ours, sd, trackers = _train_run(cuda, {"who": "pgd", "epsilon": EPS, "alpha": ALPHA, "steps": K}, fed, C)

    ref = ResNet50(C, C, False)
    ref.load_state_dict(sd)
    ref = ref.to(cuda)
    opt = optim.Adam(ref, lr=1e-3)
    loss = EntropicOpensetLoss(C, 1.0)
    mj, ma = L.AverageMeter(), L.AverageMeter()
    js, jas = [], []
    for x, y in batches:
        ref.train()
        opt.zero_grad()
        xi = x.clone().requires_grad_()
        j = loss(ref(xi)[0], y)
        j.backward()                                       # step 1 rides on the clean training backward
        g1 = ref._flat_grads.clone()
        xn = A.pgd_step(x, xi.grad, x, ALPHA, EPS)
        for p in ref.parameters():                         # steps 2..K: running statistics, input-only
            p.requires_grad_(False)
        ref.eval()
        for _ in range(K - 1):
            xk = xn.clone().requires_grad_()
            loss(ref(xk)[0], y).backward()
            xn = A.pgd_step(xn, xk.grad, x, ALPHA, EPS)
        for p in ref.parameters():
            p.requires_grad_(True)
        ref.train()
        ja = loss(ref(xn)[0], torch.full_like(y, -1))
        ja.backward()
        with torch.no_grad():
            ref._flat_grads.copy_(g1 + ref._flat_grads)
        ref.mark_gradients_ready()
        opt.step()
        js.append(j.detach())
        jas.append(ja.detach())
    for v, va, (_, y) in zip(torch.stack(js).cpu().tolist(), torch.stack(jas).cpu().tolist(), batches):
        mj.update(v, y.shape[0])
        ma.update(va, y.shape[0])
    assert _meter(trackers["j"]) == _meter(mj), "trackers['j']"
    assert _meter(trackers["j_adv"]) == _meter(ma), "trackers['j_adv']"
    assert ours.training
    assert bool((ours._nbt == 2 * STEPS).all()) and torch.equal(ours._nbt, ref._nbt)     # two training-mode forwards per step, whatever K is
    assert torch.equal(ours._flat_buffers, ref._flat_buffers), "running statistics"
    for (name, off, numel, _) in ours._pinfo:
        assert torch.equal(ours._flat_params[off:off + numel], ref._flat_params[off:off + numel]), name


def test_train_pgd_one_step_of_epsilon_is_fgsm(cuda):
    C = 10
    batches = _train_batches(cuda, C, 2)
    a, _, ta = _train_run(cuda, {"who": "fgsm", "epsilon": EPS}, batches, C)
    b, _, tb = _train_run(cuda, {"who": "pgd", "epsilon": EPS, "alpha": EPS, "steps": 1}, batches, C)
    assert torch.equal(a._flat_params, b._flat_params) and torch.equal(a._flat_buffers, b._flat_buffers) and torch.equal(a._nbt, b._nbt)
    assert _meter(ta["j"]) == _meter(tb["j"]) and _meter(ta["j_adv"]) == _meter(tb["j_adv"])


class _RecordingSync:
    """stand-in for dp's gradient sync at world size 1: the model takes its stage-by-stage path; records what it is handed"""

    def __init__(self):
        self.events = []

    def bucket_ready(self, flat, lo, hi, handoff=None):
        self.events.append(("bucket", flat.data_ptr(), lo, hi))

    def finish(self):
        self.events.append(("finish",))


def test_inner_steps_are_invisible_to_the_gradient_sync(cuda):
    """under the data-parallel stage-by-stage path a who: pgd step hands the sync exactly what a who: fgsm step hands it, and gives
    the bits of the single-call path"""
    from openset_imagenet import EntropicOpensetLoss
    from openset_imagenet.util import NameSpace
    B, HW, C = 8, 64, 10
    model, _ = _model(cuda, C, 81)
    gen = torch.Generator().manual_seed(83)
    x = torch.rand(B, 3, HW, HW, generator=gen).to(cuda)
    y = torch.randint(-1, C, (B,), generator=gen).to(cuda)
    loss = EntropicOpensetLoss(C, 1.0)
    loss3 = lambda lg, ft, t: loss(lg, t)
    snap = _snap(model)
    plans = {who: A.Plan(NameSpace({"loss": {"type": "entropic"}, "adv": adv}))
             for who, adv in (("fgsm", {"who": "fgsm", "epsilon": EPS}), ("pgd", {"who": "pgd", "epsilon": EPS, "alpha": ALPHA, "steps": 3}))}

    def step(who):
        _restore(model, snap)
        model.train()
        model._grads_fresh = False
        A.two_pass_step(model, model, x, y, loss3, plans[who])
        torch.cuda.synchronize()
        return model._flat_grads.clone()

    g_single = step("pgd")
    events = {}
    for who in ("fgsm", "pgd"):
        model._grad_sync = sync = _RecordingSync()
        try:
            g = step(who)
        finally:
            model._grad_sync = None
        events[who] = sync.events
        if who == "pgd":
            assert torch.equal(g, g_single), "summed arena"
    first, second = model._flat_grads.data_ptr(), model._flat_grads2.data_ptr()
    want = [("bucket", first, lo, hi) for lo, hi in model.gradient_buckets()] + [("finish",)] + \
           [("bucket", second, lo, hi) for lo, hi in model.gradient_buckets()] + [("finish",)]
    assert events["fgsm"] == want
    assert events["pgd"] == want, "an inner attack pass reached the gradient sync"


@pytest.mark.parametrize("who", ["pgd", "fgsm"])
def test_validate_with_attack_equals_the_hand_loop(cuda, who):
    from openset_imagenet import EntropicOpensetLoss, losses as L, tools, train as T
    from openset_imagenet.util import NameSpace
    tools.set_device_gpu(0)
    B, HW, C = 8, 64, 10
    model, sd = _model(cuda, C, 101)
    ref = _frozen_copy(cuda, sd, C)
    gen = torch.Generator().manual_seed(103)
    batches = [(torch.rand(n, 3, HW, HW, generator=gen).to(cuda), torch.randint(-1, C, (n,), generator=gen).to(cuda)) for n in (B, B, B)]
    loss = EntropicOpensetLoss(C, 1.0)
    keys = ["j", "conf_kn", "conf_unk"]
    mk = lambda: {k: L.AverageMeter() for k in keys}
    cfg = NameSpace({"parallel": True, "batch_size": B, "loss": {"type": "entropic"},
                     "adv": {"validate": {"who": who, "epsilon": EPS, "alpha": ALPHA, "steps": 3}}})
    bufs, nbt = model._flat_buffers.clone(), model._nbt.clone()
    trackers = mk()
    T.validate(model, Loader(batches), loss, C, trackers, cfg)
    assert list(trackers) == keys + ["j_adv", "conf_kn_adv", "conf_unk_adv"]
    assert not model.training and torch.equal(model._flat_buffers, bufs) and torch.equal(model._nbt, nbt)

    steps, alpha = (3, ALPHA) if who == "pgd" else (1, EPS)
    want = {k: L.AverageMeter() for k in trackers}
    rows = {"": [], "_adv": []}
    vals = {"": [], "_adv": []}
    ref.eval()
    for x, y in batches:
        xk = x
        for _ in range(steps):
            xi = xk.clone().requires_grad_()
            loss(ref(xi)[0], y).backward()
            xk = A.pgd_step(xi.detach(), xi.grad, x, alpha, EPS)
        for suffix, images in (("", x), ("_adv", xk)):
            with torch.no_grad():
                logits, _ = ref(images)
                vals[suffix].append(loss(logits, y))
                row = torch.zeros(4, dtype=torch.float64, device=cuda)
                T._confidence_partial(logits, y, 1.0 / C, -1, 0, row)
                rows[suffix].append(row)
    for suffix in ("", "_adv"):
        acc = [0.0] * 4
        for v, c, (_, y) in zip(torch.stack(vals[suffix]).cpu().tolist(), torch.stack(rows[suffix]).cpu().tolist(), batches):
            want["j" + suffix].update(v, y.shape[0])
            for i in range(4):
                acc[i] += c[i]
        if acc[1]:
            want["conf_kn" + suffix].update(acc[0] / acc[1], int(acc[1]))
        if acc[3]:
            want["conf_unk" + suffix].update(acc[2] / acc[3], int(acc[3]))
    assert {k: _meter(m) for k, m in trackers.items()} == {k: _meter(m) for k, m in want.items()}
    assert trackers["j_adv"].avg > trackers["j"].avg, "the attack ascends the loss"
    # without the block: today's keys, and the values of the plain loop on the same data
    plain = mk()
    T.validate(model, Loader(batches), loss, C, plain, NameSpace({"parallel": True, "batch_size": B, "loss": {"type": "entropic"}}))
    assert list(plain) == keys
    assert {k: _meter(m) for k, m in plain.items()} == {k: _meter(want[k]) for k in keys}


# ---- 4. uint8-staged batches: the anchor is the batch the executor staged ----------------------------------------------------------------
def _u8_case(cuda, seed, B=8, HW=64, C=10):
    gen = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, HW, HW, 3), generator=gen, dtype=torch.uint8)
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)               # every byte value is there
    y = torch.randint(-1, C, (B,), generator=gen).to(cuda)
    x = u8.permute(0, 3, 1, 2).float().div(255).contiguous().to(cuda)      # the NCHW batch u8 / 255 (true division, on the host)
    return u8.to(cuda), x, y


def test_as_nhwc4_of_a_device_uint8_batch_is_the_staged_batch(cuda):
    """value / 255 correctly rounded for all 256 byte values (a multiply by the rounded reciprocal is one ulp off for about half of
    them), and the very batch the executor stages: an FGSM step of epsilon 0 hands that batch back"""
    from openset_imagenet import EntropicOpensetLoss
    C = 10
    u8, x, y = _u8_case(cuda, 111)
    got = A.as_nhwc4(u8)
    assert got.is_cuda and got.shape == (8, 64, 64, 4) and got.is_contiguous()
    assert torch.equal(got, _nhwc4(x))
    assert torch.equal(got.cpu(), A.as_nhwc4(u8.cpu()))
    model, _ = _model(cuda, C, 113)
    model.eval()
    loss = EntropicOpensetLoss(C, 1.0)
    model.next_backward(fgsm=0.0, input_only=True)
    loss(model(u8)[0], y).backward()
    torch.cuda.synchronize()
    assert torch.equal(model.adversarial_batch(), got), "as_nhwc4(uint8) is not the batch the executor staged"
    # epsilon = 0 around that anchor returns the staged batch, whatever the step
    model.next_backward(pgd=(ALPHA, 0.0, got), input_only=True)
    loss(model(u8)[0], y).backward()
    torch.cuda.synchronize()
    assert torch.equal(model.adversarial_batch(), got)


def test_pgd_attack_train_and_validate_take_uint8_batches(cuda):
    """a uint8 batch staged on the device gives the bits of the NCHW batch u8 / 255 through pgd_attack, train() and validate()"""
    from openset_imagenet import EntropicOpensetLoss, losses as L, tools, train as T
    from openset_imagenet.util import NameSpace
    tools.set_device_gpu(0)
    C = 10
    u8, x, y = _u8_case(cuda, 121)
    loss = EntropicOpensetLoss(C, 1.0)
    loss3 = lambda lg, ft, t: loss(lg, t)
    model, _ = _model(cuda, C, 123)
    for kw in (dict(), dict(random_start=True)):
        outs = []
        for images in (u8, x):
            if kw:
                kw["generator"] = torch.Generator(device=cuda).manual_seed(9)
            outs.append(A.pgd_attack(model, images, y, loss3, EPS, ALPHA, 3, **kw).clone())
        assert torch.equal(outs[0], outs[1]), kw
        inside = outs[0][..., :3].permute(0, 3, 1, 2)
        assert bool((inside >= torch.clamp(x - EPS, min=0.0)).all()) and bool((inside <= torch.clamp(x + EPS, max=1.0)).all())
    # train(): who = pgd, three steps
    adv = {"who": "pgd", "epsilon": EPS, "alpha": ALPHA, "steps": 3}
    a, _, ta = _train_run(cuda, adv, [(u8, y)], C)
    b, _, tb = _train_run(cuda, adv, [(x, y)], C)
    assert torch.equal(a._flat_params, b._flat_params) and torch.equal(a._flat_buffers, b._flat_buffers)
    assert _meter(ta["j"]) == _meter(tb["j"]) and _meter(ta["j_adv"]) == _meter(tb["j_adv"])
    # validate(): adv.validate
    cfg = NameSpace({"parallel": True, "batch_size": 8, "loss": {"type": "entropic"},
                     "adv": {"validate": {"who": "pgd", "epsilon": EPS, "alpha": ALPHA, "steps": 2}}})
    runs = []
    for images in (u8, x):
        trackers = {k: L.AverageMeter() for k in ("j", "conf_kn", "conf_unk")}
        T.validate(model, Loader([(images, y)]), loss, C, trackers, cfg)
        runs.append({k: _meter(m) for k, m in trackers.items()})
    assert len(runs[0]) == 6 and runs[0] == runs[1]

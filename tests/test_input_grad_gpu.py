"""GPU: dJ/dimage in training mode (ABI 8) — the stem input-gradient kernel against torch fp64, the whole network's x.grad against
the fp64 oracle under the HIP path's own ReLU / arg-max decisions, the parameter gradients of a step that also produces x.grad,
the input-only backward (frozen parameters), the data-parallel stage-by-stage order, and the NHWC4 error path."""
import ctypes
import math

import pytest
import torch

from openset_imagenet import _native as N

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-4        # rel-L2, the bar of the 162 parameter gradients (tests/test_gate_pinned_gpu.py)
STEM_TAIL = ("resnet_base.conv1.weight", "resnet_base.bn1.weight", "resnet_base.bn1.bias")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. kernel parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(128, 224, 224), (64, 224, 224), (4, 225, 231), (8, 96, 128), (2, 32, 32)])
def test_stem_dgrad_kernel_vs_fp64(cuda, B, H, W):
    gen = torch.Generator().manual_seed(B * 1000 + H + W)
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = torch.randn(64, 3, 7, 7, generator=gen) * 0.1                       # OIHW
    dy = torch.randn(B, 64, Hs, Ws, generator=gen)                          # NCHW
    w_krsc3 = w.permute(0, 2, 3, 1).contiguous().to(cuda)
    dy_nhwc = dy.permute(0, 2, 3, 1).contiguous().to(cuda)
    outs = []
    for _ in range(2):
        dx = torch.full((B, 3, H, W), float("nan"), device=cuda)
        N.check(N.lib().osi_stem_dgrad(N.ptr(dy_nhwc), N.ptr(w_krsc3), N.ptr(dx), B, H, W, _stream()), "osi_stem_dgrad")
        torch.cuda.synchronize()
        outs.append(dx)
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    got = outs[0].cpu()
    assert torch.isfinite(got).all(), "an element of dx was not written"
    del dy_nhwc, outs
    ref = torch.nn.grad.conv2d_input((B, 3, H, W), w.double(), dy.double(), stride=2, padding=3)
    K = 64 * 49
    bound = (2e-6 + 6e-8 * math.sqrt(K)) * float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    print(f"stem dgrad B={B} {H}x{W}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ---- helpers for the whole-network tests -----------------------------------------------------------------------------------
def _setup(cuda, B, H, W, C, seed):
    from openset_imagenet import ResNet50
    from oracle import resnet50_oracle as R
    gen = torch.Generator().manual_seed(seed)
    sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), generator=gen)
    model = ResNet50(C, C, False)
    model.load_state_dict(sd)
    model = model.to(cuda).train()
    x = torch.rand(B, 3, H, W, generator=gen)
    wl = torch.randn(B, C, generator=gen)
    wf = torch.randn(B, C, generator=gen) * 0.1
    return model, sd, x, wl, wf


def _loss(logits, feats, wl, wf):
    return (logits * wl.to(logits.dtype)).sum() + (feats * wf.to(feats.dtype)).sum()


def _snapshot_running(model):
    return model._flat_buffers.clone(), model._nbt.clone()


def _restore_running(model, snap):
    with torch.no_grad():
        model._flat_buffers.copy_(snap[0])
        model._nbt.copy_(snap[1])


def _step(model, x, wl, wf, want_x, snap):
    """one seeded training step from the same running statistics: (x.grad or None, {name: grad copy})"""
    _restore_running(model, snap)
    xi = x.clone().requires_grad_(want_x)
    logits, feats = model(xi)
    _loss(logits, feats, wl.to(x.device), wf.to(x.device)).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return (xi.grad.detach().clone() if want_x else None), grads


# ---- 2. whole network, training mode, against the fp64 oracle -----------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,seed", [(8, 96, 96, 30, 3), (6, 75, 91, 152, 7), (4, 224, 224, 30, 13)])
def test_image_grad_vs_fp64_oracle_under_the_hip_gates(cuda, B, H, W, C, seed):
    from oracle import resnet50_oracle as R
    from osi_testlib import hip_gates
    model, sd, x, wl, wf = _setup(cuda, B, H, W, C, seed)
    snap = _snapshot_running(model)
    xg = x.to(cuda).requires_grad_()
    logits, feats = model(xg)
    loss = _loss(logits, feats, wl.to(cuda), wf.to(cuda))
    (gx_ag,) = torch.autograd.grad(loss, xg)
    torch.cuda.synchronize()
    gates = hip_gates(model)
    assert xg.grad is None
    # the same step through .backward(): x.grad gets the same bits as torch.autograd.grad
    gx, _ = _step(model, x.to(cuda), wl, wf, True, snap)
    assert torch.equal(gx, gx_ag)

    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    lg, ft = R.forward(sd64, x64, True, gates=gates)
    (ref,) = torch.autograd.grad(_loss(lg, ft, wl, wf), x64)
    got = gx.cpu()
    assert got.shape == (B, 3, H, W) and torch.isfinite(got).all()
    e = _rel(got, ref)
    per = [_rel(got[i], ref[i]) for i in range(B)]
    print(f"x.grad B={B} {H}x{W}: rel-L2 {e:.2e} overall, worst image {max(per):.2e}")
    assert e <= GRAD_TOL
    assert max(per) <= GRAD_TOL


# ---- 3. + 4. same step, same parameter gradients; input-only --------------------------------------------------------------
def test_parameter_grads_unchanged_and_input_only(cuda):
    from oracle import resnet50_oracle as R
    from osi_testlib import hip_gates
    B, H, W, C = 8, 96, 96, 30
    model, sd, x, wl, wf = _setup(cuda, B, H, W, C, 17)
    snap = _snapshot_running(model)
    xd = x.to(cuda)
    _, plain = _step(model, xd, wl, wf, False, snap)
    gates = hip_gates(model)
    gx, with_x = _step(model, xd, wl, wf, True, snap)
    assert len(plain) == 162 and plain.keys() == with_x.keys()
    for k in plain:
        if k in STEM_TAIL:
            continue
        assert torch.equal(plain[k], with_x[k]), f"{k} changed bits when x.grad was also requested"
    # the stem tail now takes the materialising branch (another summation order): close, and inside the fp64 bar
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    ref = R.forward_backward(sd64, x.double(), None, lambda lg, t, f: _loss(lg, f, wl, wf), gates=gates)[3]
    for k in STEM_TAIL:
        assert _rel(with_x[k], plain[k]) <= 1e-4, k
        assert _rel(with_x[k].cpu(), ref[k]) <= GRAD_TOL, k
    # a plain backward after the input-gradient step reproduces the plain step's bits: no state leaks
    _, again = _step(model, xd, wl, wf, False, snap)
    for k in plain:
        assert torch.equal(plain[k], again[k]), f"{k}: plain step not reproduced after an input-gradient step"

    # input-only: every parameter frozen
    for p in model.parameters():
        p.requires_grad_(False)
        p.grad = None
    sentinel = 12345.0
    model._flat_grads.fill_(sentinel)
    lib = N.lib()
    # the default schedule first (weight-gradient side stream live): nothing reaches the arena, same x.grad bits
    gx_only, none = _step(model, xd, wl, wf, True, snap)
    assert not none and all(p.grad is None for p in model.parameters())
    assert bool((model._flat_grads == sentinel).all()), "the gradient arena was written by an unprofiled input-only backward"
    assert torch.equal(gx_only, gx), "input-only x.grad differs from the full step's"
    # then under the executor's op log: no weight-gradient op at all
    _restore_running(model, snap)
    xi = xd.clone().requires_grad_()
    logits, feats = model(xi)
    net = model._last[0]
    N.check(lib.osi_resnet50_profile(net.h, 1), "profile on")
    try:
        _restore_running(model, snap)
        xi = xd.clone().requires_grad_()
        logits, feats = model(xi)
        _loss(logits, feats, wl.to(cuda), wf.to(cuda)).backward()
        ms = (ctypes.c_double * 7)()
        ops = (ctypes.c_int * 7)()
        N.check(lib.osi_resnet50_profile_read(net.h, ms, ops), "profile_read")
    finally:
        N.check(lib.osi_resnet50_profile(net.h, 0), "profile off")
    torch.cuda.synchronize()
    assert ops[3] == 0, f"{ops[3]} weight-gradient ops in an input-only backward"    # OSI_PROF_CONV_WGRAD
    assert ops[2] > 0
    assert all(p.grad is None for p in model.parameters())
    assert bool((model._flat_grads == sentinel).all()), "the gradient arena was written by an input-only backward"
    assert torch.equal(xi.grad, gx), "input-only x.grad differs from the full step's"


# ---- 3b. the project's fused losses (their plain .backward() has a direct route into the network) -----------------------------
@pytest.mark.parametrize("kind", ["entropic", "softmax", "garbage", "objectosphere"])
def test_fused_losses_fill_image_grad_and_run_input_only(cuda, kind):
    from openset_imagenet import EntropicOpensetLoss, GarbageLoss, ObjectosphereLoss, SoftmaxLoss
    B, H, W, C = 8, 64, 96, 12
    model, sd, x, wl, wf = _setup(cuda, B, H, W, C, 29)
    gen = torch.Generator().manual_seed(31)
    y = torch.randint(-1 if kind in ("entropic", "objectosphere") else 0, C, (B,), generator=gen).to(cuda)
    if kind == "entropic":
        fn = lambda lg, f: EntropicOpensetLoss(C, 1.0)(lg, y)
    elif kind == "softmax":
        fn = lambda lg, f: SoftmaxLoss()(lg, y)
    elif kind == "garbage":
        cw = (0.5 + torch.rand(C, generator=gen)).to(cuda)
        fn = lambda lg, f: GarbageLoss(cw)(lg, y)
    else:
        fn = lambda lg, f: ObjectosphereLoss(C, 1.0, 2.0, 0.1)(lg, y, f)
    snap = _snapshot_running(model)
    xd = x.to(cuda)

    def run(want_x, route):
        _restore_running(model, snap)
        xi = xd.clone().requires_grad_(want_x)
        logits, feats = model(xi)
        j = fn(logits, feats)
        if route == "plain":
            j.backward()
            gx = xi.grad if want_x else None
        else:
            (gx,) = torch.autograd.grad(j, xi)
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        return (None if gx is None else gx.detach().clone()), grads

    _, plain = run(False, "plain")                        # the direct route of the reference loop
    gx, with_x = run(True, "plain")
    assert gx is not None, "x.grad not set by the fused loss's backward()"
    gx_ag, _ = run(True, "autograd")
    assert torch.equal(gx, gx_ag), "fused-loss backward() and torch.autograd.grad give different x.grad bits"
    assert len(plain) == 162
    for k in plain:
        if k not in STEM_TAIL:
            assert torch.equal(plain[k], with_x[k]), k
        else:
            assert _rel(with_x[k], plain[k]) <= 1e-4, k

    for p in model.parameters():
        p.requires_grad_(False)
        p.grad = None
    sentinel = -777.0
    model._flat_grads.fill_(sentinel)
    model._grads_fresh = False                            # as optimizer.zero_grad() leaves it
    gx_only, none = run(True, "plain")                    # default schedule
    assert not none and all(p.grad is None for p in model.parameters())
    assert not model._grads_fresh, "an input-only backward marked the gradient arena as fresh"
    assert bool((model._flat_grads == sentinel).all()), "an input-only fused-loss backward wrote the gradient arena"
    assert torch.equal(gx_only, gx)
    net = model._last[0]
    lib = N.lib()
    N.check(lib.osi_resnet50_profile(net.h, 1), "profile on")
    try:
        gx_prof, _ = run(True, "plain")
        ms = (ctypes.c_double * 7)()
        ops = (ctypes.c_int * 7)()
        N.check(lib.osi_resnet50_profile_read(net.h, ms, ops), "profile_read")
    finally:
        N.check(lib.osi_resnet50_profile(net.h, 0), "profile off")
    assert ops[3] == 0, f"{ops[3]} weight-gradient ops in an input-only fused-loss backward"
    assert torch.equal(gx_prof, gx)
    assert bool((model._flat_grads == sentinel).all())


# ---- 5. staged (data-parallel order) --------------------------------------------------------------------------------------
class _NoComm:
    """stand-in for dp's gradient sync at world size 1: the model takes its stage-by-stage path"""

    def __init__(self):
        self.buckets = 0

    def bucket_ready(self, flat, lo, hi, handoff=None):
        self.buckets += 1

    def finish(self):
        pass


def test_staged_backward_same_bits_and_state_rule(cuda):
    B, H, W, C = 4, 64, 96, 20
    model, sd, x, wl, wf = _setup(cuda, B, H, W, C, 23)
    snap = _snapshot_running(model)
    xd = x.to(cuda)
    gx_single, g_single = _step(model, xd, wl, wf, True, snap)
    model._grad_sync = sync = _NoComm()
    try:
        gx_staged, g_staged = _step(model, xd, wl, wf, True, snap)
        assert sync.buckets == model._n_stages
        for p in model.parameters():
            p.requires_grad_(False)
        gx_only, _ = _step(model, xd, wl, wf, True, snap)
        assert sync.buckets == model._n_stages           # input-only: nothing goes to the all-reduce
    finally:
        model._grad_sync = None
    assert torch.equal(gx_single, gx_staged)
    assert torch.equal(gx_single, gx_only)
    for k in g_single:
        assert torch.equal(g_single[k], g_staged[k]), k

    # a later stage that changes the request is refused (OSI_ERR_STATE) and the backward can still be finished correctly
    lib = N.lib()
    _restore_running(model, snap)
    for p in model.parameters():
        p.requires_grad_(True)
    logits, feats = model(xd.clone().requires_grad_())
    net = model._last[0]
    dl = wl.to(cuda).contiguous()
    df = wf.to(cuda).contiguous()
    d1 = torch.empty(B, 3, H, W, device=cuda)
    d2 = torch.empty(B, 3, H, W, device=cuda)
    args = lambda dimage, pg, s: (net.h, N.ptr(model._flat_params), N.ptr(model._flat_grads), N.ptr(model._ws), N.ptr(dl), N.ptr(df),
                                  N.ptr(dimage) if dimage is not None else None, pg, s, s + 1, _stream())
    bex = lib.osi_resnet50_backward_ex
    assert bex(*args(d1, 1, 0)) == 0
    assert bex(*args(d2, 1, 1)) == -3
    assert bex(*args(None, 1, 1)) == -3
    assert bex(*args(d1, 0, 1)) == -3
    for s in range(1, model._n_stages):
        assert bex(*args(d1, 1, s)) == 0
    torch.cuda.synchronize()
    assert torch.equal(d1, gx_single)


# ---- 6. error path ----------------------------------------------------------------------------------------------------------
def test_nhwc4_batch_requiring_grad_raises(cuda):
    from openset_imagenet import ResNet50
    model = ResNet50(10, 10, False).to(cuda).train()
    x4 = torch.rand(2, 64, 64, 4, device=cuda).requires_grad_()
    with pytest.raises(ValueError, match="NCHW"):
        model(x4)
    # the torch op checks dimage's geometry against the executor's
    x = torch.rand(2, 3, 64, 64, device=cuda)
    logits, feats = model(x)
    net = model._last[0]
    bad = torch.empty(2, 3, 64, 32, device=cuda)
    with pytest.raises(RuntimeError, match="dimage"):
        N.ops().resnet50_backward_ex(net.h.value, model._flat_params, model._flat_grads, model._ws, torch.ones_like(logits), None, bad,
                                     True, 0, model._n_stages)

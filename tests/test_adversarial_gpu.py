"""GPU: adversarial negatives (ABI 10). The new path is, bit for bit, a composition of pieces that are already held to fp64 elsewhere
(tests/test_input_grad_gpu.py, the gate-pinned gradient tests), so almost every check here is torch.equal:
  3. osi_stem_dgrad_fgsm against fgsm_attack of what osi_stem_dgrad writes, and its signs against fp64;
  4. osi_resnet50_backward_adv against osi_resnet50_backward_ex(dimage) + fgsm_attack, staged, state / argument rules, the three input forms;
  5. the accumulating backward: arena = g1 + g2, the fused optimizers step on it as on a hand-summed arena;
  6. train() with cfg.adv against a loop written out of the existing public pieces;
  7. the data-parallel stage-by-stage order with a recording stand-in for the gradient sync."""
import ctypes
import math

import pytest
import torch

from openset_imagenet import _native as N
from openset_imagenet import adversary as A

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
EPS = 8.0 / 255.0


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc4(x, lane3=0.0):
    """NCHW [B, 3, H, W] -> NHWC4 [B, H, W, 4] with the 4th lane set to `lane3`"""
    B, _, H, W = x.shape
    out = torch.full((B, H, W, 4), float(lane3), device=x.device, dtype=x.dtype)
    out[..., :3] = x.permute(0, 2, 3, 1)
    return out


# ---- 3. kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(128, 224, 224), (64, 224, 224), (4, 225, 231), (8, 96, 128), (2, 32, 32)])
def test_stem_dgrad_fgsm_kernel(cuda, B, H, W):
    """Bit-equal to fgsm_attack of osi_stem_dgrad's own dx; against fp64 the adversarial pixel must be the fp64 gradient's choice
    everywhere except where |dx_fp64| is below the kernel's own error bound (a sign cannot be asked for there); that excluded share
    must stay <= 1e-4 of the elements. The fp64 twin takes its SIGN from the fp64 gradient and applies the fp32 formula to it."""
    gen = torch.Generator().manual_seed(B * 1000 + H + W)
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = torch.randn(64, 3, 7, 7, generator=gen) * 0.1
    dy = torch.randn(B, 64, Hs, Ws, generator=gen)
    x = torch.rand(B, 3, H, W, generator=gen)
    w_krsc3 = w.permute(0, 2, 3, 1).contiguous().to(cuda)
    dy_nhwc = dy.permute(0, 2, 3, 1).contiguous().to(cuda)
    xd = x.to(cuda)
    x4 = _nhwc4(xd, lane3=0.5)                             # whatever the clean batch holds in its 4th lane, x_adv's is zero
    lib = N.lib()
    dx = torch.full((B, 3, H, W), float("nan"), device=cuda)
    N.check(lib.osi_stem_dgrad(N.ptr(dy_nhwc), N.ptr(w_krsc3), N.ptr(dx), B, H, W, _stream()), "osi_stem_dgrad")
    ref = torch.nn.grad.conv2d_input((B, 3, H, W), w.double(), dy.double(), stride=2, padding=3)
    thr = (2e-6 + 6e-8 * math.sqrt(64 * 49)) * float(ref.abs().max())
    excluded = ref.abs() <= thr
    share = float(excluded.double().mean())
    sign64 = torch.sign(ref).float()
    for eps in (EPS, 0.0):
        outs = []
        for _ in range(2):
            out = torch.full((B, H, W, 4), float("nan"), device=cuda)
            N.check(lib.osi_stem_dgrad_fgsm(N.ptr(dy_nhwc), N.ptr(w_krsc3), N.ptr(x4), N.ptr(out), eps, 0.0, 1.0, B, H, W, _stream()),
                    "osi_stem_dgrad_fgsm")
            torch.cuda.synchronize()
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), "two calls differ"
        got = outs[0]
        assert torch.isfinite(got).all(), "an element of x_adv was not written"
        want = _nhwc4(A.fgsm_attack(xd, dx, eps))
        assert torch.equal(got, want), f"eps={eps}: x_adv is not fgsm_attack(x, osi_stem_dgrad's dx)"
        assert bool((got[..., 3] == 0).all())
        if eps == 0.0:
            assert torch.equal(got[..., :3], x4[..., :3])
        twin = A.fgsm_attack(x, sign64, eps)
        diff = got[..., :3].permute(0, 3, 1, 2).cpu() != twin
        outside = int((diff & ~excluded).sum())
        print(f"stem dgrad fgsm B={B} {H}x{W} eps={eps:.4f}: excluded share {share:.2e} (|dx64| <= {thr:.3e}), "
              f"{int(diff.sum())} pixels differ from the fp64 twin, {outside} of them outside the excluded set")
        assert outside == 0
    assert share <= 1e-4


# ---- helpers for the whole-network tests -----------------------------------------------------------------------------------------
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
    """the 162 tensors of two gradient arenas, bit for bit, every element written (the arenas are NaN-prefilled; the alignment gaps
    between tensors are nobody's to write)"""
    assert len(model._pinfo) == 162
    for (name, off, numel, _) in model._pinfo:
        assert torch.isfinite(a[off:off + numel]).all(), f"{name}: not written"
        assert torch.equal(a[off:off + numel], b[off:off + numel]), name


# ---- 4. executor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW", [(8, 64), (128, 224)])
def test_backward_adv_against_backward_ex_and_fgsm_attack(cuda, B, HW):
    C = 10
    model, _ = _model(cuda, C, 41)
    lib = N.lib()
    gen = torch.Generator().manual_seed(43)
    u8 = torch.randint(0, 256, (B, HW, HW, 3), generator=gen, dtype=torch.uint8)
    x = u8.permute(0, 3, 1, 2).float().div(255).contiguous().to(cuda)     # the NCHW batch u8 / 255 (true division, on the host)
    y = torch.randint(-1, C, (B,), generator=gen).to(cuda)
    snap = _snap(model)
    S = model._n_stages
    P = model._flat_params

    def forward(image):
        _restore(model, snap)
        logits, _ = model(image)
        return model._last[0], _entropic_dlogits(logits, y, C)

    # the yardstick: backward_ex with dimage and parameter gradients, then fgsm_attack of that dimage
    net, dl = forward(x)
    g_ex = torch.full_like(model._flat_grads, float("nan"))
    dimage = torch.empty(B, 3, HW, HW, device=cuda)
    assert lib.osi_resnet50_backward_ex(net.h, N.ptr(P), N.ptr(g_ex), N.ptr(model._ws), N.ptr(dl), None, N.ptr(dimage), 1, 0, S, _stream()) == 0
    torch.cuda.synchronize()
    want = _nhwc4(A.fgsm_attack(x, dimage, EPS))

    def adv(xa, g, eps, lo, s0, s1):
        return lib.osi_resnet50_backward_adv(net.h, N.ptr(P), N.ptr(g), N.ptr(model._ws), N.ptr(dl), None, N.ptr(xa), eps, lo, 1.0, s0, s1, _stream())

    # (a) + (b) one call
    net2, dl2 = forward(x)
    assert net2 is net and torch.equal(dl2, dl)
    g_adv = torch.full_like(g_ex, float("nan"))
    xa = torch.full((B, HW, HW, 4), float("nan"), device=cuda)
    assert adv(xa, g_adv, EPS, 0.0, 0, S) == 0
    torch.cuda.synchronize()
    _same_grads(model, g_adv, g_ex)                        # parameter gradients of backward_ex(dimage, param_grads = 1)
    assert torch.equal(xa, want), "x_adv is not fgsm_attack of backward_ex's dimage"

    # (c) stage by stage; a later stage with another request is refused and the backward can still be finished
    forward(x)
    g_st = torch.full_like(g_ex, float("nan"))
    xa_st = torch.full_like(xa, float("nan"))
    other = torch.empty_like(xa)
    assert adv(xa_st, g_st, EPS, 0.0, 0, 1) == 0
    assert adv(other, g_st, EPS, 0.0, 1, 2) == ERR_STATE
    assert adv(xa_st, g_st, EPS / 2, 0.0, 1, 2) == ERR_STATE
    assert adv(xa_st, g_st, EPS, -1.0, 1, 2) == ERR_STATE
    assert lib.osi_resnet50_backward(net.h, N.ptr(P), N.ptr(g_st), N.ptr(model._ws), N.ptr(dl), None, 1, 2, _stream()) == ERR_STATE
    for s in range(1, S):
        assert adv(xa_st, g_st, EPS, 0.0, s, s + 1) == 0
    torch.cuda.synchronize()
    _same_grads(model, g_st, g_ex)
    assert torch.equal(xa_st, want)

    # (d) the equal NHWC4 batch bound in place: x_adv = the bound input is refused, then the same bits
    x4 = _nhwc4(x)
    net4, dl4 = forward(x4)
    assert net4 is net and torch.equal(dl4, dl)
    g4 = torch.full_like(g_ex, float("nan"))
    assert adv(x4, g4, EPS, 0.0, 0, S) == ERR_ARG
    assert adv(model._ws.view(torch.float32)[1024:], g4, EPS, 0.0, 0, S) == ERR_ARG      # inside the workspace
    xa4 = torch.full_like(xa, float("nan"))
    assert adv(xa4, g4, EPS, 0.0, 0, S) == 0
    torch.cuda.synchronize()
    _same_grads(model, g4, g_ex)
    assert torch.equal(xa4, want)
    assert torch.equal(x4, _nhwc4(x)), "the bound clean batch was written"

    # the uint8 batch staged on the device, against the NCHW batch u8 / 255
    net8, dl8 = forward(u8.to(cuda))
    assert net8 is net and torch.equal(dl8, dl)
    g8 = torch.full_like(g_ex, float("nan"))
    xa8 = torch.full_like(xa, float("nan"))
    assert adv(xa8, g8, EPS, 0.0, 0, S) == 0
    torch.cuda.synchronize()
    _same_grads(model, g8, g_ex)
    assert torch.equal(xa8, want)


def test_torch_op_checks_x_adv_geometry(cuda):
    model, _ = _model(cuda, 10, 5)
    x = torch.rand(2, 3, 64, 64, device=cuda)
    logits, _ = model(x)
    net = model._last[0]
    bad = torch.empty(2, 64, 32, 4, device=cuda)
    with pytest.raises(RuntimeError, match="x_adv"):
        N.ops().resnet50_backward_adv(net.h.value, model._flat_params, model._flat_grads, model._ws, torch.ones_like(logits), None, bad,
                                      EPS, 0.0, 1.0, 0, model._n_stages)
    with pytest.raises(RuntimeError, match="grad_accumulate"):
        N.ops().grad_accumulate(model._flat_grads, model._flat_grads[:1024])


# ---- 5. accumulation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["adam", "sgd"])
def test_accumulating_backward_and_optimizer_step(cuda, opt_name):
    from openset_imagenet import EntropicOpensetLoss, optim
    B, HW, C = 8, 64, 10
    model, _ = _model(cuda, C, 51)
    gen = torch.Generator().manual_seed(53)
    x1, x2 = (torch.rand(B, 3, HW, HW, generator=gen).to(cuda) for _ in range(2))
    y1, y2 = (torch.randint(-1, C, (B,), generator=gen).to(cuda) for _ in range(2))
    loss = EntropicOpensetLoss(C, 1.0)
    make = (lambda: optim.Adam(model, lr=1e-3)) if opt_name == "adam" else (lambda: optim.SGD(model, lr=1e-2, momentum=0.9))
    p0 = model._flat_params.clone()
    snap = _snap(model)

    def plain(x, y):
        _restore(model, snap)
        loss(model(x)[0], y).backward()
        torch.cuda.synchronize()
        return model._flat_grads.clone()

    g1, g2 = plain(x1, y1), plain(x2, y2)
    assert not torch.equal(g1, g2)
    # the two-backward form
    opt = make()
    opt.zero_grad()
    assert not model._grads_fresh
    with pytest.raises(RuntimeError, match="accumulate"):   # nothing to add to yet
        model.next_backward(accumulate=True)
        loss(model(x1)[0], y1).backward()
    _restore(model, snap)
    loss(model(x1)[0], y1).backward()
    assert model._grads_fresh
    model.next_backward(accumulate=True)
    loss(model(x2)[0], y2).backward()
    torch.cuda.synchronize()
    assert model._grads_fresh
    assert torch.equal(model._flat_grads, g1 + g2), "arena is not g1 + g2 (one fp32 add per element)"
    for (name, off, numel, _), p in zip(model._pinfo, model._plist):
        assert p.grad is not None and p.grad.data_ptr() == model._flat_grads.data_ptr() + 4 * off, name
    # the request is consumed: the next backward overwrites again
    _restore(model, snap)
    loss(model(x2)[0], y2).backward()
    assert torch.equal(model._flat_grads, g2)
    model.next_backward(accumulate=True)
    loss(model(x1)[0], y1).backward()
    assert torch.equal(model._flat_grads, g2 + g1)
    opt.step()
    torch.cuda.synchronize()
    stepped = model._flat_params.clone()
    assert not torch.equal(stepped, p0)
    # a step on the hand-summed arena
    with torch.no_grad():
        model._flat_params.copy_(p0)
    opt2 = make()
    opt2.zero_grad()
    with torch.no_grad():
        model._flat_grads.copy_(g1 + g2)
    model.mark_gradients_ready()
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(model._flat_params, stepped)


# ---- 6. the loop ---------------------------------------------------------------------------------------------------------------------
class Loader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = range(sum(int(y.shape[0]) for _, y in batches))


def _meter(m):
    return [m.val, m.avg, m.sum, m.count]


def _loop_case(cuda, who, kind, layout):
    from openset_imagenet import EntropicOpensetLoss, GarbageLoss, ObjectosphereLoss, ResNet50, losses as L, optim, tools
    from openset_imagenet.train import train
    from openset_imagenet.util import NameSpace
    tools.set_device_gpu(0)
    B, HW, C, STEPS = 8, 64, 10, 3
    eps, std = EPS, 0.1
    gen = torch.Generator().manual_seed(61)
    batches = [(torch.rand(B, 3, HW, HW, generator=gen).to(cuda),
                torch.randint(0 if kind == "garbage" else -1, C, (B,), generator=gen).to(cuda)) for _ in range(STEPS)]
    cw = (0.5 + torch.rand(C, generator=gen)).to(cuda)
    if kind == "entropic":
        loss_fn = EntropicOpensetLoss(C, 1.0)
    elif kind == "garbage":
        loss_fn = GarbageLoss(cw)
    else:
        loss_fn = ObjectosphereLoss(C, 1.0, 2.0, 0.1)
    call = (lambda lg, ft, t: loss_fn(lg, t, ft)) if kind == "objectosphere" else (lambda lg, ft, t: loss_fn(lg, t))
    neg = C - 1 if kind == "garbage" else -1

    ours, sd = _model(cuda, C, 67)
    cfg = NameSpace({"parallel": True, "batch_size": B, "loss": {"type": kind},
                     "adv": {"who": who, "epsilon": eps, "std": std, "mu": 1.0, "decay": 0, "min_epsilon": 0.0}})
    if who != "fgsm":
        cfg.adv.generator = torch.Generator(device=cuda).manual_seed(99)
    fed = [(_nhwc4(x), y) for x, y in batches] if layout == "nhwc4" else batches
    trackers = {"j": L.AverageMeter(), "j_adv": L.AverageMeter()}
    train(ours, Loader(fed), optim.Adam(ours, lr=1e-3), loss_fn, trackers, cfg)
    torch.cuda.synchronize()

    # the same steps out of existing public pieces only
    ref = ResNet50(C, C, False)
    ref.load_state_dict(sd)
    ref = ref.to(cuda)
    opt = optim.Adam(ref, lr=1e-3)
    g = torch.Generator(device=cuda).manual_seed(99)
    mj, ma = L.AverageMeter(), L.AverageMeter()
    js, jas = [], []
    for x, y in batches:
        ref.train()
        opt.zero_grad()
        xi = x.clone().requires_grad_(who == "fgsm")
        lg, ft = ref(xi)
        j = call(lg, ft, y)
        j.backward()
        g1 = ref._flat_grads.clone()
        if who == "fgsm":
            xn = A.fgsm_attack(x, xi.grad, eps)
        elif who == "gaussian":
            xn = (x + std * torch.randn(x.shape, generator=g, device=cuda)).clamp(0.0, 1.0)
        else:
            xn = (x + eps * (2.0 * torch.rand(x.shape, generator=g, device=cuda) - 1.0)).clamp(0.0, 1.0)
        lg2, ft2 = ref(xn)
        ja = call(lg2, ft2, torch.full_like(y, neg))
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
    return ours, ref, trackers, mj, ma, 2 * STEPS


def _assert_same_run(ours, ref, trackers, mj, ma, nbt):
    assert _meter(trackers["j"]) == _meter(mj), "trackers['j']"
    assert _meter(trackers["j_adv"]) == _meter(ma), "trackers['j_adv']"
    assert bool((ours._nbt == nbt).all()) and torch.equal(ours._nbt, ref._nbt)
    assert torch.equal(ours._flat_buffers, ref._flat_buffers), "running statistics"
    for (name, off, numel, _) in ours._pinfo:
        assert torch.equal(ours._flat_params[off:off + numel], ref._flat_params[off:off + numel]), name


@pytest.mark.parametrize("kind", ["entropic", "garbage", "objectosphere"])
@pytest.mark.parametrize("who", ["fgsm", "gaussian", "uniform"])
def test_train_with_adversary_equals_the_hand_loop(cuda, who, kind):
    _assert_same_run(*_loop_case(cuda, who, kind, "nchw"))


@pytest.mark.parametrize("who", ["fgsm", "gaussian"])
def test_train_with_adversary_nhwc4_batches_same_bits(cuda, who):
    """the batches handed over in the prefetcher's layout: the hand loop (NCHW) is still the yardstick, so NHWC4 run == NCHW run"""
    _assert_same_run(*_loop_case(cuda, who, "entropic", "nhwc4"))


def test_train_with_adversary_uint8_batches(cuda):
    """uint8 batches staged on the device: FGSM takes them (the executor holds the input), a noise mode refuses them"""
    from openset_imagenet import EntropicOpensetLoss, losses as L, optim, tools
    from openset_imagenet.train import train
    from openset_imagenet.util import NameSpace
    tools.set_device_gpu(0)
    B, HW, C = 8, 64, 10
    gen = torch.Generator().manual_seed(71)
    u8 = torch.randint(0, 256, (B, HW, HW, 3), generator=gen, dtype=torch.uint8)
    y = torch.randint(-1, C, (B,), generator=gen).to(cuda)
    x = u8.permute(0, 3, 1, 2).float().div(255).contiguous().to(cuda)
    loss_fn = EntropicOpensetLoss(C, 1.0)
    runs = []
    for images in (u8.to(cuda), x):
        model, _ = _model(cuda, C, 73)
        cfg = NameSpace({"parallel": True, "loss": {"type": "entropic"}, "adv": {"who": "fgsm", "epsilon": EPS}})
        trackers = {"j": L.AverageMeter(), "j_adv": L.AverageMeter()}
        train(model, Loader([(images, y)]), optim.Adam(model, lr=1e-3), loss_fn, trackers, cfg)
        torch.cuda.synchronize()
        runs.append((model._flat_params.clone(), _meter(trackers["j"]), _meter(trackers["j_adv"])))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]
    model, _ = _model(cuda, C, 73)
    cfg = NameSpace({"parallel": True, "loss": {"type": "entropic"}, "adv": {"who": "gaussian", "std": 0.1}})
    with pytest.raises(ValueError, match="uint8"):
        train(model, Loader([(u8.to(cuda), y)]), optim.Adam(model, lr=1e-3), loss_fn, {"j": L.AverageMeter()}, cfg)


# ---- 7. data-parallel order without a second GPU -------------------------------------------------------------------------------------
class _RecordingSync:
    """stand-in for dp's gradient sync at world size 1: the model takes its stage-by-stage path; records what it is handed"""

    def __init__(self):
        self.events = []

    def bucket_ready(self, flat, lo, hi, handoff=None):
        self.events.append(("bucket", flat.data_ptr(), lo, hi))

    def finish(self):
        self.events.append(("finish",))


def test_staged_adversarial_step_same_bits(cuda):
    from openset_imagenet import EntropicOpensetLoss
    B, HW, C = 8, 64, 10
    model, _ = _model(cuda, C, 81)
    gen = torch.Generator().manual_seed(83)
    x = torch.rand(B, 3, HW, HW, generator=gen).to(cuda)
    y = torch.randint(-1, C, (B,), generator=gen).to(cuda)
    loss = EntropicOpensetLoss(C, 1.0)
    snap = _snap(model)

    def step():
        _restore(model, snap)
        model._grads_fresh = False
        j = loss(model(x)[0], y)
        model.next_backward(fgsm=EPS)
        j.backward()
        x_adv = model.adversarial_batch()
        ja = loss(model(x_adv)[0], torch.full_like(y, -1))
        model.next_backward(accumulate=True)
        ja.backward()
        torch.cuda.synchronize()
        return model._flat_grads.clone(), x_adv.clone()

    g_single, xa_single = step()
    model._grad_sync = sync = _RecordingSync()
    try:
        g_staged, xa_staged = step()
    finally:
        model._grad_sync = None
    S = model._n_stages
    first, second = model._flat_grads.data_ptr(), model._flat_grads2.data_ptr()
    assert first != second
    want = [("bucket", first, lo, hi) for lo, hi in model.gradient_buckets()] + [("finish",)] + \
           [("bucket", second, lo, hi) for lo, hi in model.gradient_buckets()] + [("finish",)]
    assert len(model.gradient_buckets()) == S
    assert sync.events == want
    assert torch.equal(g_staged, g_single), "summed arena"
    assert torch.equal(xa_staged, xa_single), "x_adv"

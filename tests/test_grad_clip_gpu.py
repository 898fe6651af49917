"""GPU: gradient-norm clipping and accumulation in the fused step (ABI 17).

1. The norm through the C ABI: spans with ragged tails, every alignment lane and uncovered float poisoned, against fp64 on the CPU.
2. The scalar: inactive, active, measure-only, inf and NaN elements, against torch's own fp32 expression.
3. osi_*_step_groups_dev: the bits of the host-scalar entry points called with the scalar read back.
4. Through the model: optim.Adam / SGD.step(clip_norm=) against clip_grad_norm_ + step of stock torch in fp64 on the CPU.
5. train() with opt.accumulate and opt.clip_norm against a hand-written loop, bit for bit.

Norm bound (1., 4.): |norm - ref| <= 2^-22 * ref, ref the fp64 value from the same fp32 data. The squares are exact in double, the
sums of < 2^25 non-negative double terms carry a relative error < 2^25 * 2^-53 = 2^-28, the square root and the product with
|grad_scale| one double rounding each, and the result is rounded to fp32 once: 2^-24 relative. 2^-22 leaves a factor 4.
Parameter and state bounds (4.): those of tests/test_optim_groups_gpu.py, unchanged.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
NORM_TOL = 2.0 ** -22
INF = float("inf")
POISON = 0x7FC12345           # a NaN with a payload


def _bits(t):
    return t.view(torch.int32)


def _poison(device="cpu"):
    return torch.tensor([POISON], dtype=torch.int32, device=device).view(torch.float32)


# ---- 1. the norm ---------------------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 30, 4001, 65537, 2, 300001, 1024, 999999, 5, 256 * 4, 7]


def _layout(n):
    """Tensors (begin, numel) laid out as the arena lays them out (every begin on a 16-byte unit), numel cycling through SIZES, every
    third tensor followed by a gap of whole uncovered units (one, then 300: past a 256-unit tile)."""
    if n == 16:
        return [(0, 1), (4, 3), (12, 4)]                       # unit 2 uncovered
    spans, off, k = [], 0, 0
    while off < n:
        numel = min(SIZES[k % len(SIZES)], n - off)
        spans.append((off, numel))
        off = (off + numel + 3) // 4 * 4
        if k % 3 == 2:
            off += 4 * (1 if k % 2 else 300)
        k += 1
    assert len(spans) <= 192
    return spans


def _covered(n, spans):
    mask = torch.zeros(n, dtype=torch.bool)
    for b, m in spans:
        mask[b:b + m] = True
    return mask


class _Norm:
    """osi_grad_clip_scale on one arena: the workspace is filled with 0xFF before every call (a NaN partial, should a slot be read
    that no workgroup wrote)."""

    def __init__(self, cuda, n):
        from openset_imagenet import _native as N
        self.N, self.n, self.cuda = N, n, cuda
        self.ws_bytes = int(N.lib().osi_grad_norm_workspace(n))
        assert self.ws_bytes >= 8 and self.ws_bytes % 8 == 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=cuda)
        self.out = torch.empty(2, device=cuda)

    def __call__(self, g, spans, norm_type, grad_scale, max_norm):
        import osi_testlib as T
        N = self.N
        table = (N.GradSpan * len(spans))(*[N.GradSpan(b, m) for b, m in spans]) if spans is not None else None
        self.ws.fill_(0xFF)
        self.out.copy_(_poison(self.cuda).repeat(2))
        N.check(N.lib().osi_grad_clip_scale(N.ptr(g), self.n, table, len(spans) if spans is not None else 0, norm_type, grad_scale, max_norm,
                                            N.ptr(self.ws), self.ws_bytes, N.ptr(self.out), T.S()), "osi_grad_clip_scale")
        return self.out.cpu()


@pytest.fixture(scope="module")
def arenas():
    """per n: (spans, covered mask, fp32 data on the CPU with every uncovered float poisoned, its fp64 L2 norm, its largest |x|)"""
    made = {}
    for n in (16, 4000, 2097152 + 4096):
        spans = _layout(n)
        mask = _covered(n, spans)
        x = torch.randn(n, generator=torch.Generator().manual_seed(n))
        l2 = float(x[mask].double().square().sum().sqrt())
        made[n] = (spans, mask, torch.where(mask, x, _poison()), l2, float(x[mask].abs().max()))
    return made


@pytest.mark.parametrize("n", [16, 4000, 2097152 + 4096])
def test_norm_over_spans_against_fp64(cuda, arenas, n):
    spans, mask, x, l2, amax = arenas[n]
    assert not bool(mask.all()) and any(m % 4 for _, m in spans)
    run = _Norm(cuda, n)
    g = x.to(cuda)
    for gs in (1.0, -0.5):
        out = run(g, spans, 2, gs, INF)
        got, ref = float(out[0]), abs(gs) * l2
        print(f"n={n} L2 grad_scale={gs}: {got!r} vs fp64 {ref!r}, off by {abs(got - ref) / ref / NORM_TOL:.3f} of the bound")
        assert abs(got - ref) <= NORM_TOL * ref
        assert float(out[1]) == gs                                        # max_norm = inf: measure only
        again = run(g, spans, 2, gs, INF)
        assert torch.equal(_bits(out), _bits(again)), "two calls, two answers"
    out = run(g, spans, 0, 1.0, INF)
    assert float(out[0]) == amax and float(out[1]) == 1.0                 # the maximum norm is exact
    assert torch.equal(_bits(out), _bits(run(g, spans, 0, 1.0, INF)))
    # squares beyond the fp32 range in both directions: an fp32 accumulation gives inf / 0
    for mag in (1e20, 1e-25):
        xs = torch.where(mask, x * mag, _poison())
        ref = float(xs[mask].double().square().sum().sqrt())
        got = float(run(xs.to(cuda), spans, 2, 1.0, INF)[0])
        print(f"n={n} magnitude {mag:g}: {got!r} vs {ref!r}")
        assert math.isfinite(got) and got > 0 and abs(got - ref) <= NORM_TOL * ref
    # spans == NULL: the whole arena
    clean = torch.where(mask, x, torch.zeros(()))
    ref = float(clean.double().square().sum().sqrt())
    got = float(run(clean.to(cuda), None, 2, 1.0, INF)[0])
    assert abs(got - ref) <= NORM_TOL * ref
    assert math.isnan(float(run(g, None, 2, 1.0, INF)[0]))               # ... poison included


# ---- 2. the scalar -------------------------------------------------------------------------------------------------------------------
def _torch_scalar(norm32, grad_scale, max_norm):
    """grad_scale * clamp(max_norm / (norm + 1e-6), max=1) as torch evaluates it on an fp32 norm tensor (clip_grad_norm_'s lines)"""
    coef = torch.clamp(max_norm / (norm32 + 1e-6), max=1.0)
    return torch.tensor(grad_scale, dtype=torch.float32) * coef


def _ulps(a, b):
    return abs(int(_bits(a.reshape(1))) - int(_bits(b.reshape(1))))


@pytest.mark.parametrize("norm_type", [2, 0])
def test_scalar_against_torch_fp32(cuda, arenas, norm_type):
    n = 4000
    spans, mask, x, l2, amax = arenas[n]
    run = _Norm(cuda, n)
    g = x.to(cuda)
    gs = 0.25
    norm = float(run(g, spans, norm_type, gs, INF)[0])
    out = run(g, spans, norm_type, gs, 2.0 * norm)                        # inactive
    assert float(out[0]) == norm and float(out[1]) == gs
    for frac in (0.5, 1.0 / 3.0, 0.9, 1e-3):                              # active
        out = run(g, spans, norm_type, gs, frac * norm)
        max32 = float(torch.tensor(frac * norm, dtype=torch.float32))     # what the C ABI receives
        want = _torch_scalar(out[0], gs, max32)
        print(f"norm_type={norm_type} max_norm={frac:.3g} * norm: scalar {float(out[1])!r}, torch {float(want)!r}")
        assert float(want) < gs and _ulps(out[1], want) <= 1
    out = run(g, spans, norm_type, -gs, 0.5 * norm)                       # a negative grad_scale keeps its sign
    assert float(out[0]) == norm and _ulps(out[1], _torch_scalar(out[0], -gs, float(torch.tensor(0.5 * norm, dtype=torch.float32)))) <= 1
    out = run(g, spans, norm_type, gs, 0.0)                               # max_norm = 0 is allowed by the C ABI: nothing moves
    assert float(out[1]) == 0.0
    first = spans[1][0]
    for bad, check in ((INF, lambda s: s == 0.0), (float("nan"), math.isnan)):
        xb = x.clone()
        xb[first] = bad
        out = run(xb.to(cuda), spans, norm_type, gs, 1.0)
        want = _torch_scalar(out[0], gs, 1.0)
        assert (math.isinf if bad == INF else math.isnan)(float(out[0]))
        assert check(float(out[1])) and check(float(want)), (bad, out)


# ---- 3. the _dev steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_dev_steps_give_the_bits_of_the_host_scalar_steps(cuda, kind):
    from openset_imagenet import _native as N
    import osi_testlib as T
    L = N.lib()
    n, S = 4000, 3
    cuts = [0, 1, 2, 4, 254, 257, 512, 513, 769, 1000]
    rows = [(b, e, i % 2) for i, (b, e) in enumerate(zip(cuts, cuts[1:])) if i % 3 != 1]     # every third segment left out
    seg = (N.OptSegment * len(rows))(*[N.OptSegment(*r) for r in rows])
    spans = [(4 * b, 4 * (e - b) - (i % 3)) for i, (b, e, _) in enumerate(rows)]               # ragged tails inside the segments
    covered = torch.zeros(n, dtype=torch.bool, device=cuda)
    for b, e, _ in rows:
        covered[4 * b:4 * e] = True
    assert not bool(covered.all())
    gen = torch.Generator().manual_seed(5)
    sentinel = _poison(cuda)
    start = [torch.where(covered, t.to(cuda), sentinel) for t in
             (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 0.02)]
    grads = [(torch.randn(n, generator=gen) * (0.1 + i)).to(cuda) for i in range(S)]
    dev, host = [t.clone() for t in start], [t.clone() for t in start]
    run = _Norm(cuda, n)

    def groups(i):
        if kind == "adam":      # one amsgrad group, one decoupled
            return (N.AdamGroup * 2)(N.AdamGroup(1e-3, 0.9, 0.999, 1e-8, 1e-2, i + 1, 0, 1, 0), N.AdamGroup(3e-3, 0.8, 0.99, 1e-6, 5e-2, i + 1, 1, 0, 0))
        return (N.SgdGroup * 2)(N.SgdGroup(1e-2, 0.9, 0.0, 1e-4, 1, int(i == 0), 0), N.SgdGroup(1e-3, 0.5, 0.5, 0.0, 0, int(i == 0), 1))

    for i, g in enumerate(grads):
        out = run(g, spans, 2, 0.5, 0.3)                                   # active: the norms are > 1
        s = float(out[1])
        assert 0.0 < s < 0.5
        scalar = N.ptr(run.out) + 4
        if kind == "adam":
            N.check(L.osi_adam_step_groups_dev(N.ptr(dev[0]), N.ptr(g), N.ptr(dev[1]), N.ptr(dev[2]), N.ptr(dev[3]), n, seg, len(rows), groups(i), 2,
                                               scalar, T.S()))
            N.check(L.osi_adam_step_groups(N.ptr(host[0]), N.ptr(g), N.ptr(host[1]), N.ptr(host[2]), N.ptr(host[3]), n, seg, len(rows), groups(i), 2,
                                           s, T.S()))
        else:
            N.check(L.osi_sgd_step_groups_dev(N.ptr(dev[0]), N.ptr(g), N.ptr(dev[1]), n, seg, len(rows), groups(i), 2, scalar, T.S()))
            N.check(L.osi_sgd_step_groups(N.ptr(host[0]), N.ptr(g), N.ptr(host[1]), n, seg, len(rows), groups(i), 2, s, T.S()))
        torch.cuda.synchronize()
    for name, a, b, t0 in zip(("param", "state 1", "state 2", "state 3"), dev, host, start):
        assert torch.equal(_bits(a), _bits(b)), f"{kind}: {name} differs from the host-scalar step"
        assert bool((_bits(a)[~covered] == POISON).all()), f"{kind}: {name} was touched outside every segment"
        if kind == "adam" or name in ("param", "state 1"):
            assert not torch.equal(_bits(a)[covered], _bits(t0)[covered]), f"{kind}: {name} did not move"


# ---- 4. through the model ----------------------------------------------------------------------------------------------------------
C = 10


@pytest.fixture(scope="module")
def net(cuda):
    from openset_imagenet import ResNet50
    torch.manual_seed(3)
    return ResNet50(C, C, False).to(cuda)


def _param_excess(p, p64, steps):
    """max over elements of |p - p64| / (2 * S * 2^-23 * max(|p64|, 1)); within the bound when <= 1"""
    bound = 2 * steps * ULP * p64.detach().double().abs().clamp(min=1.0)
    return float(((p.detach().double().cpu() - p64.detach().double()).abs() / bound).max())


def _state_rel(s, s64):
    return float((s.detach().double().cpu() - s64.detach().double()).abs().max()) / (float(s64.abs().max()) + 1e-300)


class _Twin:
    """Stock torch optimizer on the CPU (fp64, or fp32: torch's own arithmetic on the same inputs) over clones of the fused
    optimizer's parameters, group by group."""

    def __init__(self, opt, stock, dtype=torch.float64):
        self.pairs, self.dtype = [], dtype
        groups = []
        for g in opt.param_groups:
            clones = [p.detach().cpu().to(dtype).clone().requires_grad_(True) for p in g["params"]]
            self.pairs += list(zip(g["params"], clones))
            groups.append(dict({k: v for k, v in g.items() if k != "params"}, params=clones))
        self.opt = stock(groups)

    def clip_and_step(self, max_norm, norm_type):
        for p, t in self.pairs:
            t.grad = None if p.grad is None else p.grad.detach().cpu().to(self.dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_([t for _, t in self.pairs], max_norm, norm_type)
        self.opt.step()
        return float(norm)


def _backward(net, cuda, gen):
    from openset_imagenet import EntropicOpensetLoss
    x = torch.rand(2, 3, 64, 64, generator=gen).to(cuda)
    y = torch.randint(-1, C, (2,), generator=gen).to(cuda)
    net.train()
    logits, _ = net(x)
    EntropicOpensetLoss(C)(logits, y).backward()


def _grad_norm64(params, norm_type=2.0):
    gs = [p.grad.detach().double().cpu().flatten() for p in params if p.grad is not None]
    return float(torch.linalg.vector_norm(torch.cat(gs), norm_type))


@pytest.mark.parametrize("kind,norm_type", [("adam", 2.0), ("sgd", 2.0), ("adamw", INF)])
def test_clipped_steps_against_torch_fp64(net, cuda, kind, norm_type):
    """Two clipped steps; the fp64 CPU twin runs clip_grad_norm_ then step. The same inputs through torch's own fp32 path first: the
    bounds must hold for it, or the inputs are unfit (another seed, never a wider bound)."""
    from openset_imagenet import optim
    S = 2
    if kind == "sgd":
        opt = optim.SGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
        stock, keys = torch.optim.SGD, ("momentum_buffer",)
    elif kind == "adamw":
        opt = optim.AdamW(optim.split_decay(net, 1e-2), lr=1e-3)
        stock, keys = torch.optim.AdamW, ("exp_avg", "exp_avg_sq")
    else:
        opt = optim.Adam(net.parameters(), lr=1e-3)                        # the "plain" layout: clipped, it takes the grouped launch
        stock, keys = torch.optim.Adam, ("exp_avg", "exp_avg_sq")
    twin, twin32 = _Twin(opt, stock), _Twin(opt, stock, torch.float32)
    gen = torch.Generator().manual_seed(31)
    for step in range(S):
        opt.zero_grad()
        _backward(net, cuda, gen)
        raw = _grad_norm64(net.parameters(), norm_type)
        max_norm = 0.25 * raw                                              # active
        opt.step(clip_norm=max_norm, norm_type=norm_type)
        n64 = twin.clip_and_step(max_norm, norm_type)
        twin32.clip_and_step(max_norm, norm_type)
        got = opt.grad_norm
        assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
        print(f"{kind} step {step}: grad_norm {float(got)!r}, twin {n64!r}, off by {abs(float(got) - n64) / n64 / NORM_TOL:.3f} of the bound")
        assert abs(float(got) - n64) <= NORM_TOL * n64
    fit = max(_param_excess(t32, t64, S) for (_, t32), (_, t64) in zip(twin32.pairs, twin.pairs))
    worst = max(_param_excess(p, t, S) for p, t in twin.pairs)
    print(f"{kind}: worst parameter error {worst:.2f} of the bound (torch's own fp32 path on these inputs: {fit:.2f})")
    assert fit <= 1.0, "unfit inputs: torch's fp32 clip-and-step leaves the bound on them"
    assert worst <= 1.0
    for (p, t), (_, t32) in zip(twin.pairs, twin32.pairs):
        for key in keys:
            ref = twin.opt.state[t].get(key)
            if ref is not None:
                assert _state_rel(twin32.opt.state[t32][key], ref) <= 1e-5, "unfit inputs"
                rel = _state_rel(opt.state[p][key], ref)
                assert rel <= 1e-5, f"{key}: rel diff {rel:.2e}"


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_loose_clip_gives_the_bits_of_the_unclipped_step(net, cuda, kind):
    from openset_imagenet import optim
    make = (lambda: optim.Adam(net.parameters(), lr=1e-3)) if kind == "adam" else (lambda: optim.SGD(net.parameters(), lr=1e-2, momentum=0.9))
    state = "exp_avg" if kind == "adam" else "momentum_buffer"
    opt = make()
    opt.zero_grad()
    _backward(net, cuda, torch.Generator().manual_seed(32))
    p0 = net.flat_parameters().clone()
    g0 = net.flat_gradients().clone()
    results = []
    for kw in (dict(), dict(clip_norm=INF), None):
        opt = make()
        if kw is None:
            kw = dict(clip_norm=2.0 * norm)                               # twice the measured norm
        opt.step(**kw)
        if "clip_norm" in kw and kw["clip_norm"] == INF:
            norm = float(opt.grad_norm)
            assert abs(norm - _grad_norm64(net.parameters())) <= NORM_TOL * norm
        assert (opt.grad_norm is None) == (not kw)
        results.append((net.flat_parameters().clone(), opt._flat_state[state].clone()))
        with torch.no_grad():
            net.flat_parameters().copy_(p0)
    assert torch.equal(net.flat_gradients(), g0), "the gradient arena is left as the backward wrote it"
    assert not torch.equal(results[0][0], p0)
    for p, s in results[1:]:
        assert torch.equal(_bits(p), _bits(results[0][0])) and torch.equal(_bits(s), _bits(results[0][1]))


def test_norm_is_taken_over_the_tensors_the_step_updates(net, cuda):
    """a head-only optimizer: its norm is the head's while the backbone's gradients sit in the arena; a requires_grad = False tensor
    is left out, whatever its slice of the arena holds"""
    from openset_imagenet import optim
    head = list(net.logits.parameters())
    opt = optim.SGD(head, lr=1e-3)
    opt.zero_grad()
    _backward(net, cuda, torch.Generator().manual_seed(33))
    before = net.flat_parameters().clone()
    ref, everything = _grad_norm64(head), _grad_norm64(net.parameters())
    assert everything > 1.01 * ref
    opt.step(clip_norm=0.5 * ref)
    assert abs(float(opt.grad_norm) - ref) <= NORM_TOL * ref
    moved = net.flat_parameters() != before
    for (name, off, numel, shape), p in zip(net._pinfo, net._plist):
        assert bool(moved[off:off + numel].any()) == any(p is q for q in head), name

    frozen = list(net.resnet_base.layer1.parameters())
    opt = optim.Adam(net.parameters(), lr=1e-3)
    for p in frozen:
        p.requires_grad_(False)
    try:
        opt.zero_grad()
        _backward(net, cuda, torch.Generator().manual_seed(34))
        assert all(p.grad is None for p in frozen)
        slices = {id(p): (off, numel) for (name, off, numel, shape), p in zip(net._pinfo, net._plist)}
        with torch.no_grad():
            for p in frozen:                                              # whatever the frozen slices held, it is not counted
                off, numel = slices[id(p)]
                net.flat_gradients()[off:off + numel] = float("nan")
        ref = _grad_norm64(net.parameters())
        kept = [p.detach().clone() for p in frozen]
        opt.step(clip_norm=0.5 * ref)
        assert abs(float(opt.grad_norm) - ref) <= NORM_TOL * ref
        assert all(torch.equal(p.detach(), k) for p, k in zip(frozen, kept))
        assert bool(torch.isfinite(net.flat_parameters()).all())
    finally:
        for p in frozen:
            p.requires_grad_(True)


# ---- 5. the loop ---------------------------------------------------------------------------------------------------------------------
class Loader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = range(sum(int(y.shape[0]) for _, y in batches))


def _meter(m):
    return [m.val, m.avg, m.sum, m.count]


@pytest.mark.parametrize("who", [None, "fgsm"])
@pytest.mark.parametrize("opt_name", ["adam", "sgd"])
def test_train_accumulating_and_clipping_equals_the_hand_loop(cuda, opt_name, who):
    from openset_imagenet import EntropicOpensetLoss, ResNet50, losses as L, optim, tools
    from openset_imagenet.train import train
    from openset_imagenet.util import NameSpace
    from oracle import resnet50_oracle as R
    tools.set_device_gpu(0)
    B, HW, STEPS, K, EPS = 4, 64, 3, 2, 8.0 / 255.0
    gen = torch.Generator().manual_seed(41)
    batches = [(torch.rand(B, 3, HW, HW, generator=gen).to(cuda), torch.randint(-1, C, (B,), generator=gen).to(cuda)) for _ in range(STEPS)]
    sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), generator=gen)
    loss_fn = EntropicOpensetLoss(C, 1.0)
    make = (lambda m: optim.Adam(m, lr=1e-3)) if opt_name == "adam" else (lambda m: optim.SGD(m, lr=1e-2, momentum=0.9, nesterov=True))
    CLIP = 0.5      # the gradient norms of this model are of order 10 (asserted below): every step clips

    def fresh():
        m = ResNet50(C, C, False)
        m.load_state_dict(sd)
        return m.to(cuda).train()

    ours = fresh()
    d = {"parallel": True, "batch_size": B, "loss": {"type": "entropic"}, "opt": {"type": opt_name, "lr": 1e-3, "accumulate": K, "clip_norm": CLIP}}
    if who:
        d["adv"] = {"who": who, "epsilon": EPS}
    trackers = {"j": L.AverageMeter()}
    train(ours, Loader(batches), make(ours), loss_fn, trackers, NameSpace(d))
    torch.cuda.synchronize()
    assert list(trackers) == ["j"] + (["j_adv"] if who else []) + ["grad_norm"]

    ref = fresh()
    opt = make(ref)
    js, jas, norms = [], [], []
    for lo in range(0, STEPS, K):
        group = batches[lo:lo + K]
        opt.zero_grad()
        for i, (x, y) in enumerate(group):
            ref.train()
            lg, _ = ref(x)
            j = loss_fn(lg, y)
            if who or i > 0:
                ref.next_backward(fgsm=EPS if who else None, accumulate=i > 0)
            j.backward()
            js.append(j.detach())
            if who:
                lg2, _ = ref(ref.adversarial_batch())
                ja = loss_fn(lg2, torch.full_like(y, -1))
                ref.next_backward(accumulate=True)
                ja.backward()
                jas.append(ja.detach())
        opt.step(grad_scale=1.0 / len(group), clip_norm=CLIP)
        norms.append(opt.grad_norm)
    mj, ma, mn = L.AverageMeter(), L.AverageMeter(), L.AverageMeter()
    for v, (_, y) in zip(torch.stack(js).cpu().tolist(), batches):
        mj.update(v, y.shape[0])
    for v in torch.stack(norms).cpu().tolist():
        assert v > 2 * CLIP, "the test wants an active clip"
        mn.update(v, 1)
    assert mn.count == 2
    assert _meter(trackers["j"]) == _meter(mj), "trackers['j']"
    assert _meter(trackers["grad_norm"]) == _meter(mn), "trackers['grad_norm']"
    if who:
        for v, (_, y) in zip(torch.stack(jas).cpu().tolist(), batches):
            ma.update(v, y.shape[0])
        assert _meter(trackers["j_adv"]) == _meter(ma), "trackers['j_adv']"
    nbt = (2 if who else 1) * STEPS
    assert bool((ours._nbt == nbt).all()) and torch.equal(ours._nbt, ref._nbt)
    assert torch.equal(ours._flat_buffers, ref._flat_buffers), "running statistics"
    for (name, off, numel, _) in ours._pinfo:
        assert torch.equal(_bits(ours._flat_params[off:off + numel]), _bits(ref._flat_params[off:off + numel])), name
    assert not torch.equal(ours._flat_params, fresh()._flat_params)

"""CPU: projected attacks (ABI 19, openset_imagenet/adversary.py) — the new entry points are exported, declared and refuse bad arguments
before any launch; pgd_step against a scalar-loop restatement; pgd_attack, train() with who: pgd and validate() with adv.validate on a
small torch model with BatchNorm against loops written out by hand; the sharded validation (gloo, world 2) bit-identical to world 1."""
import copy
import ctypes
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from openset_imagenet import _native as N
from openset_imagenet import adversary as A
from openset_imagenet import losses as L, tools
from openset_imagenet.train import train
from openset_imagenet.util import NameSpace

ERR_ARG, ERR_STATE = -1, -3
NEW = ("osi_stem_dgrad_pgd", "osi_resnet50_backward_attack")
INF = float("inf")


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_abi_version():
    lib = N.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "osi.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in N.declared_symbols(), s
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), f"{s} not declared in include/osi.h"
    assert re.search(r"\}\s*osi_attack\s*;", header), "osi_attack not declared in include/osi.h"
    assert [f[0] for f in N.Attack._fields_] == ["x_next", "x_anchor", "alpha", "eps", "lo", "hi"]
    assert ctypes.sizeof(N.Attack) == 2 * ctypes.sizeof(ctypes.c_void_p) + 4 * 4
    assert lib.osi_abi_version() >= 19


def test_stem_dgrad_pgd_argument_errors():
    lib = N.lib()
    f = lib.osi_stem_dgrad_pgd
    dy, w, x, a, xn = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28     # aligned fake addresses, far apart: every call is refused before a launch
    al, e = 2.0 / 255.0, 8.0 / 255.0
    # the rules of osi_stem_dgrad_fgsm
    assert f(None, w, x, a, xn, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, None, x, a, xn, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, None, a, xn, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, None, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn, al, e, 0.0, 1.0, 0, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn, al, e, 0.0, 1.0, 2, 31, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn, al, e, 0.0, 1.0, 2, 64, 16, None) == ERR_ARG
    assert f(dy + 4, w, x, a, xn, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x + 4, a, xn, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn + 8, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn, al, -1e-3, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn, al, float("nan"), 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn, al, e, 1.0, 0.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, xn, al, e, 0.0, 1.0, 4096, 224, 224, None) == ERR_ARG       # dY beyond 32-bit buffer offsets
    # the anchor: non-NULL, 16-byte aligned
    assert f(dy, w, x, None, xn, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a + 4, xn, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    # alpha finite
    for bad in (INF, -INF, float("nan")):
        assert f(dy, w, x, a, xn, bad, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    # x_next overlaps neither the iterate nor the anchor
    assert f(dy, w, x, a, x, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, x + 64, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, a, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, a, a - 64, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, x, x, al, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG


@pytest.fixture
def net():
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(h), 2, 64, 64, 16, 16, 0) == 0
    yield h
    lib.osi_resnet50_destroy(h)


def test_backward_attack_argument_errors(net):
    lib = N.lib()
    f = lib.osi_resnet50_backward_attack
    ws_bytes = lib.osi_resnet50_workspace_bytes(net)
    p, g, dl = 1 << 20, 1 << 21, 1 << 22
    ws = 1 << 40
    xn = ws + ((ws_bytes + 4095) & ~4095) + (1 << 20)         # fake, aligned, outside the (fake) workspace
    anchor = xn + (1 << 24)
    al, e = 2.0 / 255.0, 8.0 / 255.0

    def call(x_next=xn, x_anchor=anchor, alpha=al, eps=e, lo=0.0, hi=1.0, pg=1, net_=net, params=p, grads=g, wsp=ws, s0=0, s1=4, a=True):
        req = N.Attack(x_next, x_anchor, alpha, eps, lo, hi)
        return f(net_, params, grads, wsp, dl, None, ctypes.byref(req) if a else None, pg, s0, s1, None)

    assert call(net_=None) == ERR_ARG
    assert call(params=None) == ERR_ARG
    assert call(wsp=None) == ERR_ARG
    assert call(a=False) == ERR_ARG
    assert call(grads=None) == ERR_ARG                        # param_grads = 1 needs the arena ...
    assert call(grads=None, pg=0) == ERR_STATE                # ... an input-only backward does not (well-formed, but no forward has run)
    assert call(pg=2) == ERR_ARG
    assert call(x_next=None) == ERR_ARG
    assert call(x_next=xn + 4) == ERR_ARG
    assert call(x_anchor=anchor + 8) == ERR_ARG
    assert call(eps=-e) == ERR_ARG
    assert call(eps=float("nan")) == ERR_ARG
    assert call(alpha=INF) == ERR_ARG
    assert call(alpha=float("nan")) == ERR_ARG
    assert call(lo=0.5, hi=0.25) == ERR_ARG
    assert call(x_next=ws + 4096) == ERR_ARG                  # x_next inside the workspace
    assert call(x_next=ws - 64) == ERR_ARG                    # ... or running into it
    assert call(x_anchor=xn) == ERR_ARG                       # x_next is the anchor
    assert call(x_anchor=xn + 64) == ERR_ARG                  # ... or overlaps it
    assert call(s1=5) == ERR_ARG
    assert call(s0=2, s1=2) == ERR_ARG
    # well-formed (negative alpha, eps = inf, no anchor, input-only) but no forward has run: the state check, nothing launched
    assert call() == ERR_STATE
    assert call(alpha=-al, eps=INF, x_anchor=None, pg=0, grads=None) == ERR_STATE


# ---- 2. pgd_step ------------------------------------------------------------------------------------------------------------------
def _pgd_step_scalar(x, g, a, alpha, eps, lo=0.0, hi=1.0):
    """the formula element by element, each operation on fp32 scalars"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    al, e, lo, hi = f32(alpha), f32(eps), f32(lo), f32(hi)
    out = torch.empty_like(x)
    for i in range(x.numel()):
        xi, gi, ai = x.reshape(-1)[i], g.reshape(-1)[i], a.reshape(-1)[i]
        s = 1.0 if gi > 0 else (-1.0 if gi < 0 else 0.0)
        t = xi + al * s
        t = min(max(t, ai - e), ai + e)
        out.view(-1)[i] = min(hi, max(lo, t))
    return out


def test_pgd_step_is_the_formula():
    gen = torch.Generator().manual_seed(1)
    a = torch.rand(3, 3, 5, 7, generator=gen)
    eps, alpha = 8.0 / 255.0, 2.0 / 255.0
    x = (a + eps * (2.0 * torch.rand(a.shape, generator=gen) - 1.0)).clamp(0.0, 1.0)
    g = torch.randn(a.shape, generator=gen)
    g[0, 0, 0, :3] = 0.0                                   # sign 0: the pixel only gets projected
    x[1, 1, 1, 1], a[1, 1, 1, 1], g[1, 1, 1, 1] = 0.999, 0.998, 1.0      # clamps at hi
    x[2, 2, 2, 2], a[2, 2, 2, 2], g[2, 2, 2, 2] = 0.001, 0.002, -1.0     # clamps at lo
    x[0, 1, 2, 3], a[0, 1, 2, 3], g[0, 1, 2, 3] = 0.5 + eps, 0.5, 1.0    # already on the ball: the step is projected back
    for al, e in ((alpha, eps), (eps, eps), (-alpha, eps), (alpha, 0.0), (alpha, INF), (0.0, eps)):
        got = A.pgd_step(x, g, a, al, e)
        assert got.dtype == torch.float32 and got.shape == x.shape
        assert torch.equal(got, _pgd_step_scalar(x, g, a, al, e)), (al, e)
    assert got[1, 1, 1, 1] <= 1.0 and A.pgd_step(x, g, a, alpha, eps)[2, 2, 2, 2] == 0.0
    assert A.pgd_step(x, g, a, alpha, eps)[0, 1, 2, 3] == (a[0, 1, 2, 3] + torch.tensor(eps, dtype=torch.float32))
    # epsilon = 0: the anchor, clamped
    assert torch.equal(A.pgd_step(x, g, a, alpha, 0.0), a.clamp(0.0, 1.0))
    assert torch.equal(A.pgd_step(x, g, 2.0 * a - 0.5, alpha, 0.0), (2.0 * a - 0.5).clamp(0.0, 1.0))
    # alpha < 0 descends: the mirror image of the ascent without projection and clamp
    assert torch.equal(A.pgd_step(x, g, a, -alpha, INF, -9.0, 9.0), A.pgd_step(x, -g, a, alpha, INF, -9.0, 9.0))
    # anchor = x and alpha <= epsilon: fgsm_attack(alpha); epsilon = inf: for any anchor
    assert torch.equal(A.pgd_step(x, g, x, eps, eps), A.fgsm_attack(x, g, eps))
    assert torch.equal(A.pgd_step(x, g, x, alpha, eps), A.fgsm_attack(x, g, alpha))
    assert torch.equal(A.pgd_step(x, g, a, alpha, INF), A.fgsm_attack(x, g, alpha))
    assert torch.equal(A.pgd_step(x, g, a, 0.3, INF, -1.0, 2.0), x + 0.3 * torch.sign(g))
    for bad in (lambda: A.pgd_step(x, g, a, alpha, -0.1), lambda: A.pgd_step(x, g, a, INF, eps), lambda: A.pgd_step(x, g, a, alpha, eps, 1.0, 0.0),
                lambda: A.pgd_step(x, g[:2], a, alpha, eps), lambda: A.pgd_step(x, g, a[:2], alpha, eps)):
        with pytest.raises(ValueError):
            bad()


def test_as_nhwc4_layouts():
    gen = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 5, 6, generator=gen)
    x4 = A.as_nhwc4(x)
    assert x4.shape == (2, 5, 6, 4) and x4.is_contiguous() and x4.dtype == torch.float32
    assert torch.equal(x4[..., :3].permute(0, 3, 1, 2), x) and bool((x4[..., 3] == 0).all())
    assert A.as_nhwc4(x4).data_ptr() == x4.data_ptr()                      # already in the layout: no copy
    u8 = torch.randint(0, 256, (2, 5, 6, 3), generator=gen, dtype=torch.uint8)
    u4 = A.as_nhwc4(u8)
    assert torch.equal(u4[..., :3], u8.float() / 255.0) and bool((u4[..., 3] == 0).all())   # ToTensor()'s true division
    for bad in (x.double(), x[:, :2], u8[..., :2], x[0]):
        with pytest.raises(ValueError):
            A.as_nhwc4(bad)


# ---- the small torch model (the helper classes of tests/test_adversarial_cpu.py) --------------------------------------------------
class TinyNet(torch.nn.Module):
    def __init__(self, hw, feat, n_out):
        super().__init__()
        self.body = torch.nn.Linear(3 * hw * hw, feat, bias=False)
        self.bn = torch.nn.BatchNorm1d(feat)
        self.logits = torch.nn.Linear(feat, n_out)

    def forward(self, x):
        f = torch.relu(self.bn(self.body(x.flatten(1))))
        return self.logits(f), f


class Loader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = range(sum(int(y.shape[0]) for _, y in batches))


HW, FEAT, B, STEPS, C = 6, 12, 8, 3, 7
EPS, ALPHA = 0.05, 0.02


def _tiny(seed=0):
    torch.manual_seed(seed)
    model = TinyNet(HW, FEAT, C)
    with torch.no_grad():                                  # running statistics that are not the initial ones
        model.bn.running_mean.copy_(torch.randn(FEAT, generator=torch.Generator().manual_seed(50)) * 0.3)
        model.bn.running_var.copy_(torch.rand(FEAT, generator=torch.Generator().manual_seed(60)) + 0.5)
    return model


def _batches(lowest, seed=3, sizes=(B,) * STEPS):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, 3, HW, HW, generator=gen), torch.randint(lowest, C, (n,), generator=gen)) for n in sizes]


def _loss(kind):
    from oracle import losses_oracle as LO
    if kind == "entropic":
        return lambda z, y: LO.entropic_openset_loss(z, y, 1.0)
    cw = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(11))
    return torch.nn.CrossEntropyLoss(weight=cw)


def _meter(m):
    return [m.val, m.avg, m.sum, m.count]


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def _project(x, g, a, alpha, eps):
    """one projected step, written out (not pgd_step: that one is held to the scalar loop above)"""
    return torch.minimum(torch.maximum(x + alpha * g.sign(), a - eps), a + eps).clamp(0.0, 1.0)


def _hand_attack(model, x0, y, loss_fn, eps, alpha, steps, start=None):
    """K steps on a COPY of the model in eval mode, the gradient from a plain backward()"""
    ref = copy.deepcopy(model).eval()
    x = x0 if start is None else start
    for _ in range(steps):
        xi = x.clone().requires_grad_()
        loss_fn(ref(xi)[0], y).backward()
        x = _project(xi.detach(), xi.grad, x0, alpha, eps)
    return x


# ---- 3. pgd_attack ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("kind", ["entropic", "garbage"])
def test_pgd_attack_equals_the_hand_loop_and_leaves_the_model_alone(kind, training):
    tools.set_device_cpu()
    model = _tiny().train(training)
    loss_fn = _loss(kind)
    (x, y), = _batches(-1 if kind == "entropic" else 0, sizes=(B,))
    # gradients of an earlier backward: the attack must not touch them
    loss_fn(model(x)[0], y).backward()
    state = copy.deepcopy(model.state_dict())
    grads = [p.grad.clone() for p in model.parameters()]
    loss3 = lambda lg, ft, t: loss_fn(lg, t)
    for steps in (1, 3):
        got = A.pgd_attack(model, x, y, loss3, EPS, ALPHA, steps)
        assert got.shape == x.shape and not got.requires_grad
        assert torch.equal(got, _hand_attack(model, x, y, loss_fn, EPS, ALPHA, steps)), steps
        assert not torch.equal(got, x)
    # every output inside [max(lo, a - eps), min(hi, a + eps)] as fp32 evaluates the bounds
    assert bool((got >= torch.clamp(x - EPS, min=0.0)).all()) and bool((got <= torch.clamp(x + EPS, max=1.0)).all())
    # random start: reproducible from the generator, and the hand loop from the same start
    r1 = A.pgd_attack(model, x, y, loss3, EPS, ALPHA, 3, random_start=True, generator=torch.Generator().manual_seed(5))
    r2 = A.pgd_attack(model, x, y, loss3, EPS, ALPHA, 3, random_start=True, generator=torch.Generator().manual_seed(5))
    start = (x + EPS * (2.0 * torch.rand(x.shape, generator=torch.Generator().manual_seed(5)) - 1.0)).clamp(0.0, 1.0)
    assert torch.equal(r1, r2) and not torch.equal(r1, got)
    assert torch.equal(r1, _hand_attack(model, x, y, loss_fn, EPS, ALPHA, 3, start))
    assert bool((r1 >= torch.clamp(x - EPS, min=0.0)).all()) and bool((r1 <= torch.clamp(x + EPS, max=1.0)).all())
    # the model: statistics, num_batches_tracked, mode and every p.grad as they were
    assert model.training is training
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    for p, g in zip(model.parameters(), grads):
        assert torch.equal(p.grad, g)
    # the mode is restored on an exception as well
    def boom(lg, ft, t):
        raise KeyError("loss failed")
    with pytest.raises(KeyError):
        A.pgd_attack(model, x, y, boom, EPS, ALPHA, 2)
    assert model.training is training
    for bad in (dict(steps=0), dict(steps=1.5), dict(steps=True), dict(epsilon=-0.1), dict(alpha=INF)):
        kw = dict(epsilon=EPS, alpha=ALPHA, steps=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            A.pgd_attack(model, x, y, loss3, **kw)


# ---- 4. train() ---------------------------------------------------------------------------------------------------------------------
def _cfg(kind, adv):
    return NameSpace({"parallel": True, "batch_size": B, "loss": {"type": kind}, "adv": adv})


@pytest.mark.parametrize("kind", ["entropic", "garbage"])
def test_train_with_pgd_equals_the_hand_loop(kind):
    tools.set_device_cpu()
    batches = _batches(-1 if kind == "entropic" else 0)
    loss_fn = _loss(kind)
    K = 3
    ours, ref = _tiny(), _tiny()
    trackers = {"j": L.AverageMeter(), "j_adv": L.AverageMeter()}
    train(ours, Loader(batches), torch.optim.Adam(ours.parameters(), lr=1e-2), loss_fn, trackers,
          _cfg(kind, {"who": "pgd", "epsilon": EPS, "alpha": ALPHA, "steps": K}))
    assert ours.training

    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    mj, ma = L.AverageMeter(), L.AverageMeter()
    neg = -1 if kind == "entropic" else C - 1
    for x, y in batches:
        ref.train()
        ropt.zero_grad()
        xi = x.clone().requires_grad_()
        j = loss_fn(ref(xi)[0], y)
        j.backward()                                       # step 1: the clean training backward's dJ/dx
        xn = _project(x, xi.grad, x, ALPHA, EPS)
        ref.eval()                                         # steps 2..K: running statistics, no parameter gradient
        for _ in range(K - 1):
            xk = xn.clone().requires_grad_()
            g, = torch.autograd.grad(loss_fn(ref(xk)[0], y), xk)
            xn = _project(xn, g, x, ALPHA, EPS)
        ref.train()
        ja = loss_fn(ref(xn)[0], torch.full_like(y, neg))
        ja.backward()
        ropt.step()
        mj.update(j.item(), y.shape[0])
        ma.update(ja.item(), y.shape[0])
    assert _meter(trackers["j"]) == _meter(mj)
    assert _meter(trackers["j_adv"]) == _meter(ma)
    assert int(ours.bn.num_batches_tracked) == 2 * STEPS   # two training-mode forwards per step, whatever K is
    _same_state(ours, ref)


def test_train_pgd_one_step_of_epsilon_is_fgsm_and_defaults():
    tools.set_device_cpu()
    batches = _batches(-1)
    loss_fn = _loss("entropic")
    runs = []
    for adv in ({"who": "fgsm", "epsilon": EPS}, {"who": "pgd", "epsilon": EPS, "alpha": EPS, "steps": 1}):
        model = _tiny()
        trackers = {"j": L.AverageMeter(), "j_adv": L.AverageMeter()}
        train(model, Loader(batches), torch.optim.Adam(model.parameters(), lr=1e-2), loss_fn, trackers, _cfg("entropic", adv))
        runs.append((model, trackers))
    _same_state(runs[0][0], runs[1][0])
    assert _meter(runs[0][1]["j"]) == _meter(runs[1][1]["j"]) and _meter(runs[0][1]["j_adv"]) == _meter(runs[1][1]["j_adv"])
    # alpha defaults to epsilon / steps * 1.25; the scheduled epsilon scales a configured alpha by the same factor
    plan = A.Plan(_cfg("entropic", {"who": "pgd", "epsilon": 0.08, "steps": 4}))
    assert (plan.steps, plan.strength, plan.alpha) == (4, 0.08, 0.08 / 4 * 1.25)
    plan = A.Plan(_cfg("entropic", {"who": "pgd", "epsilon": 0.08, "steps": 4}), epsilon=0.04)
    assert (plan.strength, plan.alpha) == (0.04, 0.04 / 4 * 1.25)
    plan = A.Plan(_cfg("entropic", {"who": "pgd", "epsilon": 0.08, "alpha": 0.02, "steps": 4}), epsilon=0.04)
    assert (plan.strength, plan.alpha) == (0.04, 0.02 * (0.04 / 0.08))
    plan = A.Plan(_cfg("entropic", {"who": "pgd", "epsilon": 0.08, "alpha": 0.02, "steps": 4}))
    assert plan.alpha == 0.02
    assert A.who_of(_cfg("entropic", {"who": "pgd", "epsilon": 0.08, "steps": 2})) == "pgd"


def test_train_pgd_refusals_at_set_up():
    tools.set_device_cpu()

    class Never(list):
        def __iter__(self):
            raise AssertionError("the loader was touched")

    def run(cfg, loss_fn):
        model = _tiny()
        train(model, Never(), torch.optim.SGD(model.parameters(), lr=0.1), loss_fn, {"j": L.AverageMeter()}, cfg)

    ok = {"who": "pgd", "epsilon": EPS, "steps": 2}
    with pytest.raises(ValueError, match="softmax"):
        run(_cfg("softmax", ok), torch.nn.CrossEntropyLoss(ignore_index=-1))
    frozen = _cfg("entropic", ok)
    frozen.freeze_below = "layer2"
    with pytest.raises(ValueError, match="freeze_below"):
        run(frozen, _loss("entropic"))
    for bad in ({"steps": 0}, {"steps": 2.5}, {"steps": True}, {"steps": None}, {"alpha": INF}, {"alpha": "big"}, {"epsilon": -0.1}):
        adv = dict(ok)
        adv.update(bad)
        with pytest.raises(ValueError):
            run(_cfg("entropic", adv), _loss("entropic"))


# ---- 5. validate() ------------------------------------------------------------------------------------------------------------------
def _oracle_confidence(T):
    from oracle import losses_oracle as LO

    def conf_partial(logits, labels, offset, unknown_class, last_valid, row):      # metrics.confidence's sums for ONE batch (oracle)
        scores = torch.softmax(logits, dim=1)
        kc, kn, nc, nn = LO.confidence(scores, labels, offset, unknown_class, None if last_valid == 0 else last_valid)
        row += torch.tensor([kc * kn, kn, nc * nn, nn], dtype=torch.float64)
    T._confidence_partial = conf_partial
    return conf_partial


VAL_SIZES = (B,) * 4 + (3,)
VAL_KEYS = ["j", "conf_kn", "conf_unk"]


def _val_trackers():
    return {k: L.AverageMeter() for k in VAL_KEYS}


def _val_meters(tr):
    return {k: (m.val, m.avg, m.sum, m.count) for k, m in tr.items()}


@pytest.mark.parametrize("who,kind", [("pgd", "entropic"), ("pgd", "garbage"), ("fgsm", "entropic")])
def test_validate_with_attack_equals_the_hand_loop(monkeypatch, who, kind):
    from openset_imagenet import train as T
    tools.set_device_cpu()
    monkeypatch.setattr(T, "_confidence_partial", T._confidence_partial)       # restored after the test
    conf_partial = _oracle_confidence(T)
    batches = _batches(-1 if kind == "entropic" else 0, seed=13, sizes=VAL_SIZES)
    loss_fn = _loss(kind)
    model = _tiny().train()
    state = copy.deepcopy(model.state_dict())
    cfg = _cfg(kind, {"validate": {"who": who, "epsilon": EPS, "alpha": ALPHA, "steps": 3}})
    trackers = _val_trackers()
    T.validate(model, batches, loss_fn, C, trackers, cfg)
    assert list(trackers) == VAL_KEYS + ["j_adv", "conf_kn_adv", "conf_unk_adv"]
    assert not model.training
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k

    # by hand: per batch the clean and the adversarial loss and sums, folded in batch order
    steps, alpha = (3, ALPHA) if who == "pgd" else (1, EPS)
    offset, unknown, last = (0.0, C - 1, -1) if kind == "garbage" else (1.0 / C, -1, 0)
    want = {k: L.AverageMeter() for k in list(trackers)}
    acc = {"": torch.zeros(4, dtype=torch.float64), "_adv": torch.zeros(4, dtype=torch.float64)}
    ref = copy.deepcopy(model).eval()
    for x, y in batches:
        for suffix, images in (("", x), ("_adv", _hand_attack(ref, x, y, loss_fn, EPS, alpha, steps))):
            with torch.no_grad():
                logits, _ = ref(images)
                want["j" + suffix].update(loss_fn(logits, y).item(), y.shape[0])
                row = torch.zeros(4, dtype=torch.float64)
                conf_partial(logits, y, offset, unknown, last, row)
                acc[suffix] = acc[suffix] + row
    for suffix, a in acc.items():
        kn_sum, kn_count, neg_sum, neg_count = a.tolist()
        if kn_count:
            want["conf_kn" + suffix].update(kn_sum / kn_count, int(kn_count))
        if neg_count:
            want["conf_unk" + suffix].update(neg_sum / neg_count, int(neg_count))
    assert _val_meters(trackers) == _val_meters(want)
    assert trackers["j_adv"].avg > trackers["j"].avg, "the attack ascends the loss"
    assert trackers["j_adv"].count == sum(VAL_SIZES)

    # without the block: exactly today's keys and the clean values
    plain = _val_trackers()
    T.validate(model, batches, loss_fn, C, plain, _cfg(kind, {"who": "no_adv"}))
    assert list(plain) == VAL_KEYS
    assert _val_meters(plain) == {k: _val_meters(trackers)[k] for k in VAL_KEYS}
    for bad in ({"who": "gaussian"}, {"who": "pgd", "epsilon": EPS}, {"who": "pgd", "epsilon": -1.0, "steps": 2}):
        with pytest.raises(ValueError):
            T.validate(model, batches, loss_fn, C, _val_trackers(), _cfg(kind, {"validate": bad}))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _sharded_worker(rank, world, port, out):
    import sys
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path[:0] = [root, os.path.join(root, "openset-imagenet_amd")]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from openset_imagenet import train as T
        tools.set_device_cpu()
        _oracle_confidence(T)
        for kind in ("entropic", "garbage"):
            model = _tiny()
            with torch.no_grad():                     # statistics that DIFFER per rank: rank 0's model is attacked and scored everywhere
                model.bn.running_mean.add_(0.1 * rank)
            batches = _batches(-1 if kind == "entropic" else 0, seed=13, sizes=VAL_SIZES)
            loss_fn = _loss(kind)
            cfg = _cfg(kind, {"validate": {"who": "pgd", "epsilon": EPS, "alpha": ALPHA, "steps": 2}})
            sharded, single = _val_trackers(), _val_trackers()
            T.validate(model, batches[rank::world], loss_fn, C, sharded, cfg, shard=(rank, world))
            T.validate(model, batches, loss_fn, C, single, cfg)       # the whole loader in one process
            assert _val_meters(sharded) == _val_meters(single), (kind, _val_meters(sharded), _val_meters(single))
            assert len(sharded) == 6 and sharded["j_adv"].count == sum(VAL_SIZES)
            out.put((rank, kind, _val_meters(sharded)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_sharded_validation_with_attack_is_bit_identical_to_world_1():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    res = sorted(out.get(timeout=5) for _ in range(2 * world))
    for kind in ("entropic", "garbage"):
        per_rank = [m for _, k, m in res if k == kind]
        assert len(per_rank) == world and per_rank[0] == per_rank[1], "every rank ends with the same trackers"

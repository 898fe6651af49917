"""CPU: adversarial negatives (ABI 10, openset_imagenet/adversary.py) — the new entry points are exported, declared and refuse bad
arguments before any launch; fgsm_attack / noise_negatives against a literal restatement; the epsilon schedule, the negative label per
loss type, softmax refused; and train() on a small torch model: unchanged without an adversary, equal to a literal two-pass torch loop
with one."""
import ctypes
import os
import re

import pytest
import torch

from openset_imagenet import _native as N
from openset_imagenet import adversary as A
from openset_imagenet import losses as L, tools
from openset_imagenet.train import train
from openset_imagenet.util import NameSpace

ERR_ARG, ERR_STATE = -1, -3
NEW = ("osi_stem_dgrad_fgsm", "osi_grad_accumulate", "osi_resnet50_backward_adv")


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_abi_version():
    lib = N.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "osi.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in N.declared_symbols(), s
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), f"{s} not declared in include/osi.h"
    assert lib.osi_abi_version() >= 9


def test_stem_dgrad_fgsm_argument_errors():
    lib = N.lib()
    f = lib.osi_stem_dgrad_fgsm
    dy, w, x, xa = 1 << 24, 1 << 25, 1 << 26, 1 << 27     # aligned fake addresses, far apart: every call below must be refused before a launch
    e = 8.0 / 255.0
    assert f(None, w, x, xa, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, None, x, xa, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, None, xa, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, None, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, xa, e, 0.0, 1.0, 0, 64, 64, None) == ERR_ARG            # empty batch
    assert f(dy, w, x, xa, e, 0.0, 1.0, 2, 31, 64, None) == ERR_ARG            # below the executor's smallest image
    assert f(dy, w, x, xa, e, 0.0, 1.0, 2, 64, 16, None) == ERR_ARG
    assert f(dy + 4, w, x, xa, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG        # dY is read in 16-byte vectors
    assert f(dy, w, x + 4, xa, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG        # pixels are loaded ...
    assert f(dy, w, x, xa + 8, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG        # ... and stored as 16-byte vectors
    assert f(dy, w, x, xa, -1e-3, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG        # eps < 0
    assert f(dy, w, x, xa, float("nan"), 0.0, 1.0, 2, 64, 64, None) == ERR_ARG
    assert f(dy, w, x, xa, e, 1.0, 0.0, 2, 64, 64, None) == ERR_ARG            # lo > hi
    assert f(dy, w, x, x, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG             # aliased images
    assert f(dy, w, x, x + 64, e, 0.0, 1.0, 2, 64, 64, None) == ERR_ARG        # overlapping images
    assert f(dy, w, x, xa, e, 0.0, 1.0, 4096, 224, 224, None) == ERR_ARG       # dY beyond 32-bit buffer offsets


def test_grad_accumulate_argument_errors():
    lib = N.lib()
    f = lib.osi_grad_accumulate
    a, b = 1 << 24, 1 << 25
    assert f(None, b, 1024, None) == ERR_ARG
    assert f(a, None, 1024, None) == ERR_ARG
    assert f(a, b, 0, None) == ERR_ARG
    assert f(a, b, 1022, None) == ERR_ARG           # n % 4
    assert f(a + 4, b, 1024, None) == ERR_ARG       # 16-byte vectors
    assert f(a, b + 8, 1024, None) == ERR_ARG
    assert f(a, a, 1024, None) == ERR_ARG           # an arena added to itself is a caller error


@pytest.fixture
def net():
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(h), 2, 64, 64, 16, 16, 0) == 0
    yield h
    lib.osi_resnet50_destroy(h)


def test_backward_adv_argument_errors(net):
    lib = N.lib()
    f = lib.osi_resnet50_backward_adv
    ws_bytes = lib.osi_resnet50_workspace_bytes(net)
    p, g, dl = 1 << 20, 1 << 21, 1 << 22
    ws = 1 << 40
    xa = ws + ((ws_bytes + 4095) & ~4095) + (1 << 20)         # fake, aligned, outside the (fake) workspace
    e = 8.0 / 255.0
    assert f(None, p, g, ws, dl, None, xa, e, 0.0, 1.0, 0, 4, None) == ERR_ARG
    assert f(net, None, g, ws, dl, None, xa, e, 0.0, 1.0, 0, 4, None) == ERR_ARG
    assert f(net, p, None, ws, dl, None, xa, e, 0.0, 1.0, 0, 4, None) == ERR_ARG      # always a parameter-gradient backward
    assert f(net, p, g, None, dl, None, xa, e, 0.0, 1.0, 0, 4, None) == ERR_ARG
    assert f(net, p, g, ws, dl, None, None, e, 0.0, 1.0, 0, 4, None) == ERR_ARG
    assert f(net, p, g, ws, dl, None, xa + 4, e, 0.0, 1.0, 0, 4, None) == ERR_ARG
    assert f(net, p, g, ws, dl, None, xa, -e, 0.0, 1.0, 0, 4, None) == ERR_ARG
    assert f(net, p, g, ws, dl, None, xa, e, 0.5, 0.25, 0, 4, None) == ERR_ARG
    assert f(net, p, g, ws, dl, None, ws + 4096, e, 0.0, 1.0, 0, 4, None) == ERR_ARG  # x_adv inside the workspace
    assert f(net, p, g, ws, dl, None, ws - 64, e, 0.0, 1.0, 0, 4, None) == ERR_ARG    # ... or running into it
    assert f(net, p, g, ws, dl, None, xa, e, 0.0, 1.0, 0, 5, None) == ERR_ARG         # stage range
    assert f(net, p, g, ws, dl, None, xa, e, 0.0, 1.0, 2, 2, None) == ERR_ARG
    # well-formed but no forward has run: the executor's state check, still nothing launched
    assert f(net, p, g, ws, dl, None, xa, e, 0.0, 1.0, 0, 4, None) == ERR_STATE


# ---- 2. the torch-op definitions -----------------------------------------------------------------------------------------------
def test_fgsm_attack_is_the_formula():
    gen = torch.Generator().manual_seed(1)
    x = torch.rand(3, 3, 5, 7, generator=gen)
    g = torch.randn(3, 3, 5, 7, generator=gen)
    g[0, 0, 0, :3] = 0.0                                   # sign 0: the pixel stays
    x[1, 1, 1, 1], g[1, 1, 1, 1] = 0.999, 1.0              # clamps at hi
    x[2, 2, 2, 2], g[2, 2, 2, 2] = 0.001, -1.0             # clamps at lo
    eps = 8.0 / 255.0
    got = A.fgsm_attack(x, g, eps)
    want = torch.empty_like(x)
    e32 = torch.tensor(eps, dtype=torch.float32)
    for i in range(x.numel()):
        xi, gi = x.view(-1)[i], g.view(-1)[i]
        s = 1.0 if gi > 0 else (-1.0 if gi < 0 else 0.0)
        want.view(-1)[i] = min(torch.tensor(1.0), max(torch.tensor(0.0), xi + e32 * s))
    assert torch.equal(got, want)
    assert torch.equal(got[0, 0, 0, :3], x[0, 0, 0, :3]) and got[1, 1, 1, 1] == 1.0 and got[2, 2, 2, 2] == 0.0
    assert torch.equal(A.fgsm_attack(x, g, 0.0), x)
    assert torch.equal(A.fgsm_attack(x, g, 0.5, -1.0, 2.0), x + 0.5 * torch.sign(g))
    with pytest.raises(ValueError):
        A.fgsm_attack(x, g, -0.1)
    with pytest.raises(ValueError):
        A.fgsm_attack(x, g, 0.1, 1.0, 0.0)
    with pytest.raises(ValueError):
        A.fgsm_attack(x, g[:2], 0.1)


@pytest.mark.parametrize("who", ["gaussian", "uniform"])
def test_noise_negatives_layouts_and_seed(who):
    x = torch.rand(4, 3, 6, 5, generator=torch.Generator().manual_seed(2))
    got = A.noise_negatives(x, who, 0.3, torch.Generator().manual_seed(7))
    gen = torch.Generator().manual_seed(7)
    noise = torch.randn(4, 3, 6, 5, generator=gen) if who == "gaussian" else 2.0 * torch.rand(4, 3, 6, 5, generator=gen) - 1.0
    want = (x + 0.3 * noise).clamp(0.0, 1.0)
    assert torch.equal(got, want) and got.shape == x.shape
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and not torch.equal(got, x)
    # the same seed, the batch handed over as NHWC4: the same negatives in that layout, 4th lane zero
    x4 = torch.zeros(4, 6, 5, 4)
    x4[..., :3] = x.permute(0, 2, 3, 1)
    x4[..., 3] = 5.0                                        # whatever the lane held, the result's is zero
    got4 = A.noise_negatives(x4, who, 0.3, torch.Generator().manual_seed(7))
    assert got4.shape == x4.shape and got4.is_contiguous()
    assert torch.equal(got4[..., :3].permute(0, 3, 1, 2), want)
    assert bool((got4[..., 3] == 0).all())
    with pytest.raises(ValueError):
        A.noise_negatives((x4[..., :3] * 255).to(torch.uint8), who, 0.3)
    with pytest.raises(ValueError):
        A.noise_negatives(x, "fgsm", 0.3)


def test_epsilon_schedule():
    adv = NameSpace({"who": "fgsm", "epsilon": 0.4, "mu": 0.5, "decay": 2, "min_epsilon": 0.07})
    assert [A.scheduled_epsilon(adv, e) for e in range(8)] == [max(0.07, 0.4 * 0.5 ** (e // 2)) for e in range(8)]
    assert A.scheduled_epsilon(adv, 7) == 0.07
    const = NameSpace({"who": "fgsm", "epsilon": 0.4, "mu": 0.5, "decay": 0})
    assert all(A.scheduled_epsilon(const, e) == 0.4 for e in (0, 1, 50))
    assert A.scheduled_epsilon(NameSpace({"who": "fgsm", "epsilon": 0.25}), 9) == 0.25


def test_negative_label_and_refusals():
    assert A.negative_label("entropic", 10) == -1
    assert A.negative_label("objectosphere", 10) == -1
    assert A.negative_label("garbage", 10) == 9
    with pytest.raises(ValueError):
        A.negative_label("softmax", 10)
    assert A.who_of(NameSpace({"parallel": True})) == "no_adv"
    assert A.who_of(NameSpace({"adv": {"epsilon": 0.1}})) == "no_adv"
    assert A.who_of(NameSpace({"adv": {"who": "uniform"}})) == "uniform"
    with pytest.raises(ValueError):
        A.who_of(NameSpace({"adv": {"who": "pgd"}}))
    # softmax + an adversary: refused when the loop is set up, before any batch is drawn
    model, batches = _tiny(5), []
    cfg = NameSpace({"parallel": True, "loss": {"type": "softmax"}, "adv": {"who": "fgsm", "epsilon": 0.1}})

    class Never(list):
        def __iter__(self):
            raise AssertionError("the loader was touched")

    with pytest.raises(ValueError, match="softmax"):
        train(model, Never(batches), torch.optim.SGD(model.parameters(), lr=0.1), torch.nn.CrossEntropyLoss(ignore_index=-1),
              {"j": L.AverageMeter()}, cfg)


# ---- the loop on a small torch model (the helper classes of tests/test_loop_contract.py) --------------------------------------------
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


HW, FEAT, B, STEPS = 6, 12, 8, 3


def _tiny(C, seed=0):
    torch.manual_seed(seed)
    return TinyNet(HW, FEAT, C)


def _batches(C, lowest, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, HW, HW, generator=gen), torch.randint(lowest, C, (B,), generator=gen)) for _ in range(STEPS)]


def _loss(kind, C):
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


@pytest.mark.parametrize("adv", [None, {"who": "no_adv", "epsilon": 0.3}])
def test_default_loop_is_the_parent_loop(adv):
    """without an `adv` block, or with who: no_adv, train() is the loop it was: a literal copy of that loop gives the same bits"""
    C = 7
    tools.set_device_cpu()
    batches = _batches(C, 0)
    loss_fn = _loss("garbage", C)
    d = {"parallel": True, "batch_size": B, "loss": {"type": "garbage"}}
    if adv is not None:
        d["adv"] = adv
    ours, ref = _tiny(C), _tiny(C)
    opt = torch.optim.Adam(ours.parameters(), lr=1e-2)
    trackers = {"j": L.AverageMeter()}
    train(ours, Loader(batches), opt, loss_fn, trackers, NameSpace(d))
    assert list(trackers) == ["j"]
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    meter = L.AverageMeter()
    for x, y in batches:
        ref.train()
        ropt.zero_grad()
        logits, _ = ref(x)
        j = loss_fn(logits, y)
        meter.update(j.item(), y.shape[0])
        j.backward()
        ropt.step()
    assert _meter(trackers["j"]) == _meter(meter)
    _same_state(ours, ref)


@pytest.mark.parametrize("kind", ["entropic", "garbage"])
@pytest.mark.parametrize("who", ["fgsm", "gaussian", "uniform"])
def test_adversarial_loop_equals_a_literal_two_pass_loop(who, kind):
    C = 7
    tools.set_device_cpu()
    batches = _batches(C, -1 if kind == "entropic" else 0)
    loss_fn = _loss(kind, C)
    eps, std = 0.05, 0.2
    cfg = NameSpace({"parallel": True, "batch_size": B, "loss": {"type": kind},
                     "adv": {"who": who, "epsilon": 0.5, "std": std, "mu": 1.0, "decay": 0, "min_epsilon": 0.0}})
    if who != "fgsm":
        cfg.adv.generator = torch.Generator().manual_seed(99)
    ours, ref = _tiny(C), _tiny(C)
    opt = torch.optim.Adam(ours.parameters(), lr=1e-2)
    trackers = {"j": L.AverageMeter(), "j_adv": L.AverageMeter()}
    trackers["j_adv"].update(5.0, 3)                       # reset by train() like every tracker
    train(ours, Loader(batches), opt, loss_fn, trackers, cfg, epsilon=eps)     # the scheduled value wins over adv.epsilon
    assert ours.training

    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    gen = torch.Generator().manual_seed(99)
    mj, ma = L.AverageMeter(), L.AverageMeter()
    neg = -1 if kind == "entropic" else C - 1
    for x, y in batches:
        ref.train()
        ropt.zero_grad()
        xi = x.clone().requires_grad_(who == "fgsm")
        logits, _ = ref(xi)
        j = loss_fn(logits, y)
        j.backward()
        if who == "fgsm":
            xn = (x + eps * torch.sign(xi.grad)).clamp(0.0, 1.0)
        elif who == "gaussian":
            xn = (x + std * torch.randn(x.shape, generator=gen)).clamp(0.0, 1.0)
        else:
            xn = (x + eps * (2.0 * torch.rand(x.shape, generator=gen) - 1.0)).clamp(0.0, 1.0)
        logits_n, _ = ref(xn)
        ja = loss_fn(logits_n, torch.full_like(y, neg))
        ja.backward()
        ropt.step()
        mj.update(j.item(), y.shape[0])
        ma.update(ja.item(), y.shape[0])
    assert _meter(trackers["j"]) == _meter(mj)
    assert _meter(trackers["j_adv"]) == _meter(ma)
    assert int(ours.bn.num_batches_tracked) == 2 * STEPS   # both forwards update the running statistics
    _same_state(ours, ref)

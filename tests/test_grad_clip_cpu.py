"""CPU: gradient-norm clipping and accumulation (ABI 17) — the new entry points are exported and declared and refuse bad arguments
before any launch; step(clip_norm=, norm_type=) and the loop keys opt.accumulate / opt.clip_norm / opt.clip_norm_type refuse bad
values; and train() on a small torch model: with the keys it equals a literal hand-written loop (mul_, clip_grad_norm_, step) bit for
bit, with and without an adversary; without them it is the parent loop with its tracker set."""
import ctypes
import os
import re

import pytest
import torch

import openset_imagenet as oi
from openset_imagenet import _native as N
from openset_imagenet import losses as L, optim, tools
from openset_imagenet.train import step_options, train
from openset_imagenet.util import NameSpace

ERR_ARG = -1
NEW = ("osi_grad_norm_workspace", "osi_grad_clip_scale", "osi_adam_step_groups_dev", "osi_sgd_step_groups_dev")
INF = float("inf")


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_abi_version():
    lib = N.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "osi.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in N.declared_symbols(), s
        assert re.search(r"\b(int|size_t)\s+" + s + r"\s*\(", header), f"{s} not declared in include/osi.h"
    for word in ("osi_grad_span", "OSI_NORM_INF 0", "OSI_NORM_L2 2"):
        assert word in header
    assert lib.osi_abi_version() >= 17
    assert ctypes.sizeof(N.GradSpan) == 16
    assert (N.NORM_INF, N.NORM_L2) == (0, 2)


def test_workspace_follows_the_chunking():
    ws = N.lib().osi_grad_norm_workspace
    assert ws(16) == 8 and ws(4 * 256) == 8 and ws(4 * 257) == 16        # one 8-byte partial per workgroup, one workgroup per 256 units
    assert ws(4 * 256 * 2048) == 8 * 2048 and ws(4 * 256 * 2048 + 4) == 8 * 1025   # above 2048 tiles a workgroup takes two
    assert ws(0) == 0 and ws(6) == 0                                       # what the call refuses


G, WS, OUT = 1 << 24, 1 << 25, 1 << 26     # aligned fake addresses: every call below must be refused before anything is dereferenced


def _spans(rows):
    return (N.GradSpan * len(rows))(*[N.GradSpan(*r) for r in rows]), len(rows)


def _clip(n=64, spans=((0, 64),), norm=2, gs=1.0, mx=1.0, g=G, ws=WS, ws_bytes=None, out=OUT, span_ptr=True, nspans=None):
    s, ns = _spans(spans)
    wb = N.lib().osi_grad_norm_workspace(n) if ws_bytes is None else ws_bytes
    return N.lib().osi_grad_clip_scale(g, n, s if span_ptr else None, ns if nspans is None else nspans, norm, gs, mx, ws, wb, out, None)


def test_grad_clip_scale_argument_errors():
    bad = ERR_ARG
    assert _clip(g=None) == bad and _clip(ws=None) == bad and _clip(out=None) == bad
    assert _clip(g=G + 4) == bad                                                # the arena is read in 16-byte vectors
    assert _clip(n=0) == bad and _clip(n=62, spans=((0, 62),)) == bad           # n % 4 != 0
    assert _clip(n=4 * (2 ** 32 - 511), ws_bytes=1 << 20) == bad                # n / 4 beyond the grouped kernels' limit
    assert _clip(ws_bytes=7) == bad and _clip(n=4 * 257, ws_bytes=8) == bad     # workspace too small
    assert _clip(spans=((2, 8),)) == bad                                        # begin % 4
    assert _clip(spans=((0, 4), (8, 0))) == bad                                 # empty
    assert _clip(spans=((8, 4), (0, 4))) == bad                                 # unsorted
    assert _clip(spans=((0, 9), (8, 4))) == bad                                 # overlapping
    assert _clip(spans=((0, 65),)) == bad and _clip(spans=((64, 1),)) == bad    # past n
    assert _clip(spans=((60, 2 ** 64 - 8),)) == bad                             # begin + numel wraps
    assert _clip(n=4 * 200, spans=tuple((4 * i, 1) for i in range(193))) == bad  # more than 192 entries
    assert _clip(nspans=0) == bad                                               # a table with no entries
    assert _clip(span_ptr=False, nspans=1) == bad                               # NULL means n_spans == 0
    assert _clip(norm=1) == bad and _clip(norm=3) == bad and _clip(norm=-1) == bad
    assert _clip(mx=-1e-3) == bad and _clip(mx=float("nan")) == bad
    assert _clip(gs=INF) == bad and _clip(gs=-INF) == bad and _clip(gs=float("nan")) == bad


def _segs(rows):
    return (N.OptSegment * len(rows))(*[N.OptSegment(*r) for r in rows]), len(rows)


def test_dev_steps_argument_errors():
    """the refusals of osi_*_step_groups, and a null or misaligned scalar"""
    lib = N.lib()
    D = 16
    ag = (N.AdamGroup * 1)(N.AdamGroup(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0, 0))
    sg = (N.SgdGroup * 1)(N.SgdGroup(1e-2, 0.9, 0.0, 0.0, 0, 1, 0))
    adam = lambda n=64, segs=((0, 16, 0),), s=D, p=D, grp=ag: lib.osi_adam_step_groups_dev(p, D, D, D, None, n, *_segs(segs), grp, 1, s, None)
    sgd = lambda n=64, segs=((0, 16, 0),), s=D, p=D, grp=sg: lib.osi_sgd_step_groups_dev(p, D, D, n, *_segs(segs), grp, 1, s, None)
    for call in (adam, sgd):
        assert call(s=None) == ERR_ARG and call(s=D + 2) == ERR_ARG
        assert call(p=None) == ERR_ARG and call(n=62) == ERR_ARG and call(n=0) == ERR_ARG
        assert call(segs=((4, 8, 0), (0, 4, 0))) == ERR_ARG and call(segs=((0, 17, 0),)) == ERR_ARG and call(segs=((0, 4, 1),)) == ERR_ARG
        assert call(grp=None) == ERR_ARG
    assert adam(grp=(N.AdamGroup * 1)(N.AdamGroup(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0, 0))) == ERR_ARG      # step < 1
    assert adam(grp=(N.AdamGroup * 1)(N.AdamGroup(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 1, 0))) == ERR_ARG      # amsgrad without its arena
    assert sgd(grp=(N.SgdGroup * 1)(N.SgdGroup(1e-2, 0.0, 0.0, 0.0, 1, 1, 0))) == ERR_ARG                    # nesterov without momentum


# ---- 2. ValueErrors -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return oi.ResNet50(12, 12, False)


@pytest.mark.parametrize("make", [lambda m: optim.Adam(m, lr=1e-3), lambda m: optim.AdamW(m, lr=1e-3), lambda m: optim.SGD(m, lr=1e-2)],
                         ids=["adam", "adamw", "sgd"])
def test_step_refuses_bad_clip_arguments(model, make):
    opt = make(model)
    for clip in (0, 0.0, -1.0, float("nan"), "1", True):
        with pytest.raises(ValueError):
            opt.step(clip_norm=clip)
    for kind in (1, 3.0, 0, -INF, float("nan"), "inf", None):
        with pytest.raises(ValueError):
            opt.step(clip_norm=1.0, norm_type=kind)
    assert opt.grad_norm is None
    for kind in (2, 2.0, INF):
        opt.step(clip_norm=INF, norm_type=kind)        # well-formed; no backward has run, so the step is skipped
        assert opt.grad_norm is None
    opt.step()
    assert opt.grad_norm is None


def test_spans_are_the_tensors_the_step_updates(model):
    head = list(model.logits.parameters())
    opt = optim.Adam(head, lr=1e-3)
    opt._plan_for()
    info = {id(p): model._pinfo[i] for i, p in enumerate(model._plist)}
    want = sorted((info[id(p)][1], info[id(p)][2]) for p in head)
    pairs = [tuple(opt._spans[i:i + 2]) for i in range(0, len(opt._spans), 2)]
    assert sum(n for _, n in pairs) == sum(n for _, n in want) and pairs[0][0] == want[0][0]
    full = optim.SGD(model, lr=1e-2)
    full._plan_for()
    pairs = [tuple(full._spans[i:i + 2]) for i in range(0, len(full._spans), 2)]
    assert all(b % 4 == 0 and n >= 1 for b, n in pairs) and len(pairs) <= N.OPT_MAX_SEGMENTS
    assert all(b0 + n0 <= b1 for (b0, n0), (b1, _) in zip(pairs, pairs[1:]))
    assert sum(n for _, n in pairs) == sum(p.numel() for p in model.parameters())      # no alignment lane inside a span
    frozen = head[0]
    frozen.requires_grad_(False)
    try:
        opt._plan_for()
        assert sum(opt._spans[1::2]) == sum(p.numel() for p in head[1:])
    finally:
        frozen.requires_grad_(True)


def test_loop_keys_are_validated_when_the_loop_is_set_up():
    base = {"parallel": True, "loss": {"type": "garbage"}}
    assert step_options(NameSpace(base)) == (1, None, 2.0)                          # no opt block at all
    assert step_options(NameSpace(dict(base, opt={"type": "adam", "lr": 1e-3}))) == (1, None, 2.0)
    assert step_options(NameSpace(dict(base, opt={"accumulate": 4, "clip_norm": 1, "clip_norm_type": "inf"}))) == (4, 1.0, INF)
    assert step_options(NameSpace(dict(base, opt={"clip_norm": INF, "clip_norm_type": 2}))) == (1, INF, 2.0)

    class Never(list):
        def __iter__(self):
            raise AssertionError("the loader was touched")

    net = TinyNet(HW, FEAT, 5)
    for bad in ({"accumulate": 0}, {"accumulate": -2}, {"accumulate": 2.0}, {"accumulate": True}, {"accumulate": "2"},
                {"clip_norm": 0}, {"clip_norm": -1.0}, {"clip_norm": float("nan")}, {"clip_norm": "big"},
                {"clip_norm": 1.0, "clip_norm_type": 1}, {"clip_norm": 1.0, "clip_norm_type": "l2"}, {"clip_norm_type": 3}):
        with pytest.raises(ValueError):
            train(net, Never(), torch.optim.SGD(net.parameters(), lr=0.1), torch.nn.CrossEntropyLoss(), {"j": L.AverageMeter()},
                  NameSpace(dict(base, opt=bad)))


# ---- 3. the loop on a small torch model (the helper classes of tests/test_adversarial_cpu.py) -----------------------------------
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


def _tiny(seed=0):
    torch.manual_seed(seed)
    return TinyNet(HW, FEAT, C)


def _batches(lowest, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, HW, HW, generator=gen), torch.randint(lowest, C, (B,), generator=gen)) for _ in range(STEPS)]


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


CLIP = 0.05     # far below the gradient norms of this model (asserted below): every step clips


@pytest.mark.parametrize("norm_type", [2, "inf"])
@pytest.mark.parametrize("who", [None, "fgsm"])
def test_accumulating_clipping_loop_equals_a_literal_loop(who, norm_type):
    """accumulate: 2 over 3 batches (a full group and a ragged one) with an active clip_norm, on CPU with torch.optim.Adam"""
    tools.set_device_cpu()
    kind = "entropic" if who else "garbage"
    batches = _batches(-1 if who else 0)
    loss_fn = _loss(kind)
    eps = 0.05
    d = {"parallel": True, "batch_size": B, "loss": {"type": kind},
         "opt": {"type": "adam", "lr": 1e-2, "accumulate": 2, "clip_norm": CLIP, "clip_norm_type": norm_type}}
    if who:
        d["adv"] = {"who": who, "epsilon": eps}
    ours, ref = _tiny(), _tiny()
    opt = torch.optim.Adam(ours.parameters(), lr=1e-2)
    trackers = {"j": L.AverageMeter()}
    train(ours, Loader(batches), opt, loss_fn, trackers, NameSpace(d))
    assert list(trackers) == ["j"] + (["j_adv"] if who else []) + ["grad_norm"]

    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    params = list(ref.parameters())
    kind_f = INF if norm_type == "inf" else 2.0
    mj, ma, mn = L.AverageMeter(), L.AverageMeter(), L.AverageMeter()
    for lo in range(0, STEPS, 2):
        group = batches[lo:lo + 2]
        ropt.zero_grad()
        for x, y in group:
            ref.train()
            xi = x.clone().requires_grad_(bool(who))
            logits, _ = ref(xi)
            j = loss_fn(logits, y)
            j.backward()                                         # autograd adds into p.grad
            mj.update(j.item(), y.shape[0])
            if who:
                xn = (x + eps * torch.sign(xi.grad)).clamp(0.0, 1.0)
                logits_n, _ = ref(xn)
                ja = loss_fn(logits_n, torch.full_like(y, -1))
                ja.backward()
                ma.update(ja.item(), y.shape[0])
        r = len(group)
        if r > 1:
            for p in params:
                p.grad.mul_(1.0 / r)
        norm = torch.nn.utils.clip_grad_norm_(params, CLIP, kind_f)
        assert float(norm) > 2 * CLIP, "the test wants an active clip"
        mn.update(norm.item(), 1)
        ropt.step()
    assert mn.count == 2
    assert _meter(trackers["j"]) == _meter(mj)
    assert _meter(trackers["grad_norm"]) == _meter(mn)
    if who:
        assert _meter(trackers["j_adv"]) == _meter(ma)
    assert int(ours.bn.num_batches_tracked) == (2 if who else 1) * STEPS     # statistics per micro-batch
    _same_state(ours, ref)


def test_accumulate_alone_adds_no_tracker_and_clip_alone_steps_every_batch():
    tools.set_device_cpu()
    batches, loss_fn = _batches(0), _loss("garbage")
    base = {"parallel": True, "batch_size": B, "loss": {"type": "garbage"}}
    # accumulate: 3 = one step on the mean of the three gradients
    ours, ref = _tiny(), _tiny()
    trackers = {"j": L.AverageMeter()}
    train(ours, Loader(batches), torch.optim.SGD(ours.parameters(), lr=0.1, momentum=0.9), loss_fn, trackers, NameSpace(dict(base, opt={"accumulate": 3})))
    assert list(trackers) == ["j"] and trackers["j"].count == STEPS * B
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    ropt.zero_grad()
    for x, y in batches:
        ref.train()
        loss_fn(ref(x)[0], y).backward()
    for p in ref.parameters():
        p.grad.mul_(1.0 / 3)
    ropt.step()
    _same_state(ours, ref)
    # clip_norm alone: three steps, three norms; inf measures and leaves the step alone
    ours, ref = _tiny(), _tiny()
    trackers = {"j": L.AverageMeter()}
    train(ours, Loader(batches), torch.optim.SGD(ours.parameters(), lr=0.1), loss_fn, trackers, NameSpace(dict(base, opt={"clip_norm": INF})))
    assert trackers["grad_norm"].count == STEPS and trackers["grad_norm"].val > 0
    train(ref, Loader(batches), torch.optim.SGD(ref.parameters(), lr=0.1), loss_fn, {"j": L.AverageMeter()}, NameSpace(base))
    _same_state(ours, ref)


@pytest.mark.parametrize("opt_block", [None, {"type": "adam", "lr": 1e-2}, {"type": "adam", "lr": 1e-2, "accumulate": 1}])
def test_keys_absent_is_the_parent_loop(opt_block):
    tools.set_device_cpu()
    batches, loss_fn = _batches(0), _loss("garbage")
    d = {"parallel": True, "batch_size": B, "loss": {"type": "garbage"}}
    if opt_block is not None:
        d["opt"] = opt_block
    ours, ref = _tiny(), _tiny()
    opt = torch.optim.Adam(ours.parameters(), lr=1e-2)
    calls = []
    plain_step = opt.step
    opt.step = lambda *a, **k: (calls.append((a, k)), plain_step(*a, **k))[1]
    trackers = {"j": L.AverageMeter()}
    train(ours, Loader(batches), opt, loss_fn, trackers, NameSpace(d))
    assert list(trackers) == ["j"]
    assert calls == [((), {})] * STEPS                      # step() as it was called before, once per batch
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

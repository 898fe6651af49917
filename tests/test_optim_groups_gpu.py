"""GPU: the grouped optimizer kernels (k_adam_groups / k_sgd_groups) and the optimizers built on them.

1. Segment boundaries, bit-exact through the C ABI: groups with default options give the bits of the plain kernels, units outside
   every segment keep theirs.
2. Every option against stock torch.optim in fp64 on the CPU, started from the same fp32 values.
3. Through the model: group layouts, subsets, frozen parameters, state-dict exchange with torch, and the unchanged plain route.

Parameter bound (2. and 3.): per element |p - p64| <= 2 * S * 2^-23 * max(|p64|, 1) after S steps. At most three fp32 roundings
of p-sized quantities per step in the decoupled form (p * (1 - lr*wd), the fp32 value of that factor, the final subtraction):
<= 1.5 units of 2^-23 |p|, rounded up to 2. torch's own fp32 path against fp64 stays <= 2.96 units over three steps for all nine
option sets (worst: AdamW); a dropped decay term alone is about 80 units.
State bound: max|s - s64| / max|s64| <= 1e-5, the bar of test_model_gpu.test_adam_step_and_optimizer_state_dict (the fp32
reference alone gives <= 1.6e-7).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _param_excess(p, p64, steps):
    """max over elements of |p - p64| / (2 * S * 2^-23 * max(|p64|, 1)); within the bound when <= 1"""
    bound = 2 * steps * ULP * p64.abs().clamp(min=1.0)
    return float(((p.detach().double().cpu() - p64.detach()).abs() / bound).max())


def _state_rel(s, s64):
    return float((s.detach().double().cpu() - s64.detach()).abs().max()) / (float(s64.abs().max()) + 1e-300)


def _bits(t):
    return t.view(torch.int32)


# ---- 1. boundaries -------------------------------------------------------------------------------------------------------------
def _cuts(n4):
    """Segment boundaries in 16-byte units: lengths 1, 1, 2, 250, 3, 255, 1, 256, ... and, for the large arena, boundaries at
    524288 +- 1 (where the plain kernels' 2048 x 256 grid-stride loop wraps) and off the 256-unit tile grid beyond it."""
    marks = [0, 1, 2, 4, 254, 257, 512, 513, 769, 1000, 3071, 3072, 3073, 200000, 524287, 524289, 524288 + 700, n4]
    return sorted({m for m in marks if m <= n4})


def _segments(N, cuts, keep, n_groups):
    rows = [(b, e, i % n_groups) for i, (b, e) in enumerate(zip(cuts, cuts[1:])) if keep(i)]
    return (N.OptSegment * len(rows))(*[N.OptSegment(*r) for r in rows]), len(rows), rows


@pytest.mark.parametrize("n", [16, 4000, 2097152 + 4096])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_default_groups_give_the_bits_of_the_plain_kernels(cuda, kind, n):
    from openset_imagenet import _native as N
    import osi_testlib as T
    L = N.lib()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen).to(cuda)
    m0 = (torch.randn(n, generator=gen) * 0.1).to(cuda)
    v0 = (torch.rand(n, generator=gen) * 0.01).to(cuda)
    grads = [(torch.randn(n, generator=gen) * (0.1 + i)).to(cuda) for i in range(3)]
    lr, gscale, n_groups = (1e-3, 0.5, 3)
    sentinel = torch.tensor([0x7FC12345], dtype=torch.int32, device=cuda).view(torch.float32)   # a NaN with a payload

    def plain():
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        for i, g in enumerate(grads):
            if kind == "adam":
                N.check(L.osi_adam_step(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), n, lr, 0.9, 0.999, 1e-8, i + 1, gscale, T.S()))
            else:
                N.check(L.osi_sgd_step(N.ptr(p), N.ptr(g), N.ptr(m), n, lr, 0.9, int(i == 0), gscale, T.S()))
        return p, m, v

    def grouped(keep):
        cuts = _cuts(n // 4)
        seg, nseg, rows = _segments(N, cuts, keep, n_groups)
        covered = torch.zeros(n, dtype=torch.bool, device=cuda)
        for b, e, k in rows:
            covered[4 * b:4 * e] = True
        p, m, v = (torch.where(covered, t, sentinel) for t in (p0, m0, v0))
        vmax = sentinel.repeat(n)                   # no amsgrad group: never touched
        for i, g in enumerate(grads):
            if kind == "adam":
                gs = (N.AdamGroup * n_groups)(*[N.AdamGroup(lr, 0.9, 0.999, 1e-8, 0.0, i + 1, 0, 0, 0) for _ in range(n_groups)])
                N.check(L.osi_adam_step_groups(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), N.ptr(vmax), n, seg, nseg, gs, n_groups, gscale, T.S()))
            else:
                gs = (N.SgdGroup * n_groups)(*[N.SgdGroup(lr, 0.9, 0.0, 0.0, 0, int(i == 0), 0) for _ in range(n_groups)])
                N.check(L.osi_sgd_step_groups(N.ptr(p), N.ptr(g), N.ptr(m), n, seg, nseg, gs, n_groups, gscale, T.S()))
        return covered, p, m, v, vmax

    ref = plain()
    states = 3 if kind == "adam" else 2
    covered, *got = grouped(lambda i: True)
    assert bool(covered.all())
    for name, a, b in zip(("param", "state 1", "state 2")[:states], got, ref):
        assert torch.equal(_bits(a), _bits(b)), f"{kind} n={n}: {name} differs from the plain kernel"
    assert bool((_bits(got[3]) == _bits(sentinel)).all())
    covered, *got = grouped(lambda i: i % 2 == 0)            # every second segment left out
    assert not bool(covered.all())
    for name, a, b in zip(("param", "state 1", "state 2")[:states], got, ref):
        assert torch.equal(_bits(a)[covered], _bits(b)[covered]), f"{kind} n={n}: covered {name} differs from the plain kernel"
        assert bool((_bits(a)[~covered] == _bits(sentinel)).all()), f"{kind} n={n}: {name} was touched outside every segment"
    assert bool((_bits(got[3]) == _bits(sentinel)).all())


# ---- 2. options against torch fp64 -----------------------------------------------------------------------------------------
ADAM_OPTIONS = [dict(weight_decay=1e-2), dict(amsgrad=True), dict(weight_decay=1e-2, decoupled_weight_decay=True),
                dict(weight_decay=5e-2, decoupled_weight_decay=True, amsgrad=True, maximize=True),
                dict(betas=(0.8, 0.99), eps=1e-6, lr=3e-3, weight_decay=1e-3)]
SGD_OPTIONS = [dict(weight_decay=1e-4), dict(nesterov=True, weight_decay=5e-4), dict(dampening=0.5, maximize=True),
               dict(momentum=0.0, weight_decay=1e-4)]


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_options_against_torch_fp64(cuda, kind):
    from openset_imagenet import _native as N
    import osi_testlib as T
    L = N.lib()
    n, S = 4000, 3
    options = ADAM_OPTIONS if kind == "adam" else SGD_OPTIONS
    K = len(options)
    cuts = [(n // 4) * k // K for k in range(K + 1)]           # one launch, the groups side by side
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (0.1 + i) for i in range(S)]
    twin = [p0[4 * b:4 * e].double().clone().requires_grad_(True) for b, e in zip(cuts, cuts[1:])]
    make = (lambda gs: torch.optim.Adam(gs, lr=1e-3)) if kind == "adam" else (lambda gs: torch.optim.SGD(gs, lr=1e-2, momentum=0.9))
    topt = make([dict(params=[t], **o) for t, o in zip(twin, options)])
    p = p0.to(cuda)
    s1, s2, s3 = (torch.zeros(n, device=cuda) for _ in range(3))
    seg = (N.OptSegment * K)(*[N.OptSegment(b, e, k) for k, (b, e) in enumerate(zip(cuts, cuts[1:]))])
    for i, g in enumerate(grads):
        for t, (b, e) in zip(twin, zip(cuts, cuts[1:])):
            t.grad = g[4 * b:4 * e].double().clone()
        topt.step()
        gg = g.to(cuda)
        if kind == "adam":
            gs = (N.AdamGroup * K)(*[N.AdamGroup(q["lr"], q["betas"][0], q["betas"][1], q["eps"], q["weight_decay"], i + 1,
                                                 int(q["decoupled_weight_decay"]), int(q["amsgrad"]), int(q["maximize"]))
                                     for q in topt.param_groups])
            N.check(L.osi_adam_step_groups(N.ptr(p), N.ptr(gg), N.ptr(s1), N.ptr(s2), N.ptr(s3), n, seg, K, gs, K, 1.0, T.S()))
        else:
            gs = (N.SgdGroup * K)(*[N.SgdGroup(q["lr"], q["momentum"], q["dampening"], q["weight_decay"], int(q["nesterov"]), int(i == 0),
                                               int(q["maximize"])) for q in topt.param_groups])
            N.check(L.osi_sgd_step_groups(N.ptr(p), N.ptr(gg), N.ptr(s1), n, seg, K, gs, K, 1.0, T.S()))
    report, failed = [], []
    for k, (t, o, (b, e)) in enumerate(zip(twin, options, zip(cuts, cuts[1:]))):
        excess = _param_excess(p[4 * b:4 * e], t, S)
        st = topt.state[t]
        names = {"exp_avg": s1, "exp_avg_sq": s2, "max_exp_avg_sq": s3} if kind == "adam" else {"momentum_buffer": s1}
        rels = {key: _state_rel(arena[4 * b:4 * e], st[key]) for key, arena in names.items() if st.get(key) is not None}
        report.append(f"{kind} {o}: param {excess:.2f} of the bound, state {rels}")
        if excess > 1.0 or any(r > 1e-5 for r in rels.values()):
            failed.append(report[-1])
        if kind == "adam" and not o.get("amsgrad"):
            assert not bool(s3[4 * b:4 * e].any()), "max_exp_avg_sq written for a group without amsgrad"
        if kind == "sgd" and o.get("momentum", 0.9) == 0.0:
            assert "momentum_buffer" not in st or st["momentum_buffer"] is None
            assert not bool(s1[4 * b:4 * e].any()), "the buffer arena was written for a momentum-free group"
    print("\n".join(report))
    assert not failed, failed


# ---- 3. through the model ----------------------------------------------------------------------------------------------------
C = 10


@pytest.fixture(scope="module")
def net(cuda):
    from openset_imagenet import ResNet50
    torch.manual_seed(3)
    return ResNet50(C, C, False).to(cuda)


class _Twin:
    """Stock torch optimizer in fp64 on the CPU over clones of the fused optimizer's parameters, group by group."""

    def __init__(self, opt, stock, params=None):
        self.pairs = []
        groups = []
        for g in opt.param_groups:
            clones = [p.detach().cpu().double().clone().requires_grad_(True) for p in g["params"]]
            self.pairs += list(zip(g["params"], clones))
            groups.append(dict({k: v for k, v in g.items() if k != "params"}, params=clones))
        self.opt = stock(groups)

    def take_grads(self):
        for p, t in self.pairs:
            t.grad = None if p.grad is None else p.grad.detach().cpu().double().clone()

    def worst(self, steps):
        return max(_param_excess(p, t, steps) for p, t in self.pairs)


def _backward(net, cuda, gen):
    from openset_imagenet import EntropicOpensetLoss
    x = torch.rand(2, 3, 64, 64, generator=gen).to(cuda)
    y = torch.randint(-1, C, (2,), generator=gen).to(cuda)
    net.train()
    logits, _ = net(x)
    EntropicOpensetLoss(C)(logits, y).backward()


def _run(net, cuda, opt, twin, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        opt.zero_grad()
        _backward(net, cuda, gen)
        twin.take_grads()
        opt.step()
        twin.opt.step()


def _check_states(opt, twin, keys):
    for p, t in twin.pairs:
        for key in keys:
            ref = twin.opt.state[t].get(key) if t in twin.opt.state else None
            if ref is not None:
                rel = _state_rel(opt.state[p][key], ref)
                assert rel <= 1e-5, f"{key}: rel diff {rel:.2e}"


def test_adamw_split_decay_through_the_model(net, cuda):
    from openset_imagenet import optim
    opt = optim.AdamW(optim.split_decay(net, 1e-2), lr=1e-3)
    twin = _Twin(opt, torch.optim.AdamW)
    _run(net, cuda, opt, twin, 2, seed=11)
    worst = twin.worst(2)
    print(f"AdamW split_decay: worst parameter error {worst:.2f} of the bound")
    assert worst <= 1.0
    _check_states(opt, twin, ("exp_avg", "exp_avg_sq"))
    a, b = opt.state_dict(), twin.opt.state_dict()
    assert set(a["state"]) == set(b["state"]) and all(float(a["state"][i]["step"]) == float(b["state"][i]["step"]) == 2.0 for i in b["state"])


def test_sgd_nesterov_head_and_backbone_rates(net, cuda):
    from openset_imagenet import optim
    head = list(net.logits.parameters())
    body = [p for p in net.parameters() if all(p is not q for q in head)]
    opt = optim.SGD([dict(params=head, lr=1e-2), dict(params=body)], lr=1e-3, momentum=0.9, nesterov=True)
    twin = _Twin(opt, torch.optim.SGD)
    _run(net, cuda, opt, twin, 2, seed=12)
    worst = twin.worst(2)
    print(f"SGD nesterov, two rates: worst parameter error {worst:.2f} of the bound")
    assert worst <= 1.0
    _check_states(opt, twin, ("momentum_buffer",))


def test_head_only_leaves_everything_else_alone(net, cuda):
    from openset_imagenet import optim
    opt = optim.Adam(net.logits.parameters())
    twin = _Twin(opt, torch.optim.Adam)
    head = {id(p) for p in net.logits.parameters()}
    before = net.flat_parameters().clone()
    _run(net, cuda, opt, twin, 2, seed=13)
    assert twin.worst(2) <= 1.0
    touched = torch.zeros_like(before, dtype=torch.bool)
    for (name, off, numel, shape), p in zip(net._pinfo, net._plist):
        if id(p) in head:
            touched[off:off + numel] = True
            assert not torch.equal(p.detach(), net._view(before, off, numel, shape)), f"{name} was not stepped"
        else:
            assert torch.equal(p.detach(), net._view(before, off, numel, shape)), f"{name} moved"
    assert torch.equal(net.flat_parameters()[~touched], before[~touched])
    for key in ("exp_avg", "exp_avg_sq"):
        assert not bool(opt._flat_state[key][~touched].any()), f"{key} was written outside the head"
        assert bool(opt._flat_state[key][touched].any())
    assert "max_exp_avg_sq" not in opt._flat_state
    a, b = opt.state_dict(), twin.opt.state_dict()
    assert set(a["state"]) == set(b["state"]) == set(range(len(head)))
    assert all(set(a["state"][i]) == set(b["state"][i]) for i in b["state"])


def test_frozen_layer_is_skipped_and_keeps_its_own_step_count(net, cuda):
    from openset_imagenet import optim
    opt = optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-4)
    twin = _Twin(opt, torch.optim.Adam)
    frozen = list(net.resnet_base.layer1.parameters())
    assert len(frozen) >= 20
    kept = [p.detach().clone() for p in frozen]
    for p in frozen:
        p.requires_grad_(False)
    try:
        _run(net, cuda, opt, twin, 1, seed=14)
        assert all(p.grad is None for p in frozen) and all(p.grad is not None for p in net.logits.parameters())
        assert all(torch.equal(p.detach(), k) for p, k in zip(frozen, kept))
        assert len(opt._plan_for()[2]) == 1
    finally:
        for p in frozen:
            p.requires_grad_(True)
    _run(net, cuda, opt, twin, 1, seed=15)
    assert len(opt._plan_for()[2]) == 2 and not opt._plan_for()[0]     # two step-count classes inside the one user group
    assert not any(torch.equal(p.detach(), k) for p, k in zip(frozen, kept))
    a, b = opt.state_dict(), twin.opt.state_dict()
    assert set(a["state"]) == set(b["state"])
    frozen_ids = {id(p) for p in frozen}
    for i, p in enumerate(opt.param_groups[0]["params"]):
        want = 1.0 if id(p) in frozen_ids else 2.0
        assert float(a["state"][i]["step"]) == float(b["state"][i]["step"]) == want
    worst = twin.worst(2)
    print(f"frozen layer1, then unfrozen: worst parameter error {worst:.2f} of the bound")
    assert worst <= 1.0
    _check_states(opt, twin, ("exp_avg", "exp_avg_sq"))


def test_state_dicts_cross_load_with_stock_torch(net, cuda):
    from openset_imagenet import optim
    make = lambda: optim.AdamW(optim.split_decay(net, 1e-2), lr=1e-3, amsgrad=True)
    opt = make()
    twin = _Twin(opt, torch.optim.AdamW)
    _run(net, cuda, opt, twin, 2, seed=16)
    assert twin.worst(2) <= 1.0
    ours, theirs = opt.state_dict(), twin.opt.state_dict()
    opt2 = make()
    opt2.load_state_dict(theirs)                                          # torch's state into the fused optimizer
    twin.opt = torch.optim.AdamW([dict({k: v for k, v in g.items() if k != "params"}, params=g["params"]) for g in twin.opt.param_groups])
    twin.opt.load_state_dict(ours)                                        # the fused state into a fresh torch optimizer
    assert opt2._steps == 2 and "max_exp_avg_sq" in opt2._flat_state
    _run(net, cuda, opt2, twin, 1, seed=17)
    worst = twin.worst(3)
    print(f"cross-loaded state dicts, third step: worst parameter error {worst:.2f} of the bound")
    assert worst <= 1.0
    _check_states(opt2, twin, ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
    assert all(float(v["step"]) == 3.0 for v in opt2.state_dict()["state"].values())


def test_legacy_construction_still_takes_the_plain_launch(net, cuda):
    from openset_imagenet import _native as N, optim
    import osi_testlib as T
    opt = optim.Adam(net.parameters(), lr=1e-3)
    n = net.flat_parameters().numel()
    m, v = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    gen = torch.Generator().manual_seed(18)
    for step in (1, 2):
        opt.zero_grad()
        _backward(net, cuda, gen)
        p, g = net.flat_parameters().clone(), net.flat_gradients().clone()
        N.check(N.lib().osi_adam_step(N.ptr(p), N.ptr(g), N.ptr(m), N.ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, step, 1.0, T.S()))
        opt.step()
        assert torch.equal(_bits(net.flat_parameters()), _bits(p))
        assert torch.equal(_bits(opt._flat_state["exp_avg"]), _bits(m)) and torch.equal(_bits(opt._flat_state["exp_avg_sq"]), _bits(v))
    assert opt._plan_for()[0] and opt._steps == 2


def test_add_param_group_after_a_step(net, cuda):
    """Gradual unfreezing: the head alone takes a step, then the layer below joins as a group of its own (with AMSGrad, so that a
    third state arena appears late). The added parameters get state entries with their own step count, as in torch."""
    from openset_imagenet import optim
    opt = optim.Adam(net.logits.parameters(), lr=1e-3)
    twin = _Twin(opt, torch.optim.Adam)
    _run(net, cuda, opt, twin, 1, seed=19)
    added = list(net.resnet_base.fc.parameters())
    extra = dict(lr=3e-4, weight_decay=1e-3, amsgrad=True)
    opt.add_param_group(dict(extra, params=added))
    clones = [p.detach().cpu().double().clone().requires_grad_(True) for p in added]
    twin.pairs += list(zip(added, clones))
    twin.opt.add_param_group(dict(extra, params=clones))
    n_head = len(opt.param_groups[0]["params"])
    a, b = opt.state_dict(), twin.opt.state_dict()
    assert set(a["state"]) == set(b["state"]) == set(range(n_head))       # torch holds nothing for the added group before it steps
    _run(net, cuda, opt, twin, 1, seed=20)
    a, b = opt.state_dict(), twin.opt.state_dict()
    assert set(a["state"]) == set(b["state"]) == set(range(n_head + len(added)))
    for i in b["state"]:
        assert set(a["state"][i]) == set(b["state"][i])
        assert float(a["state"][i]["step"]) == float(b["state"][i]["step"]) == (2.0 if i < n_head else 1.0)
    worst = twin.worst(2)
    print(f"add_param_group after a step: worst parameter error {worst:.2f} of the bound")
    assert worst <= 1.0
    _check_states(opt, twin, ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
    fresh = lambda cls, params: cls([dict({k: v for k, v in g.items() if k != "params"}, params=ps)
                                     for g, ps in zip(opt.param_groups, params)])
    opt2 = fresh(optim.Adam, [g["params"] for g in opt.param_groups])
    opt2.load_state_dict(b)                                               # torch's state into a fresh fused optimizer
    twin.opt = fresh(torch.optim.Adam, [g["params"] for g in twin.opt.param_groups])
    twin.opt.load_state_dict(a)                                           # the fused state into a fresh torch optimizer
    _run(net, cuda, opt2, twin, 1, seed=21)
    worst = twin.worst(3)
    print(f"add_param_group after a step, cross-loaded, one more step: worst parameter error {worst:.2f} of the bound")
    assert worst <= 1.0
    _check_states(opt2, twin, ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
    steps = [float(v["step"]) for v in opt2.state_dict()["state"].values()]
    assert steps == [3.0] * n_head + [2.0] * len(added)

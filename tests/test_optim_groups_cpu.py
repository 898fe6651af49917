"""CPU: the grouped optimizer steps (osi_adam_step_groups / osi_sgd_step_groups) are exported and declared and refuse malformed
tables before any launch; the fused optimizers accept torch.optim-style group layouts over one model's arena, build the segment
table the kernels walk, and keep the state-dict schema of the stock torch optimizers."""
import ctypes

import pytest
import torch

import openset_imagenet as oi
from openset_imagenet import _native as N, optim


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return oi.ResNet50(12, 12, False)


def _segs(rows):
    return (N.OptSegment * len(rows))(*[N.OptSegment(*r) for r in rows]), len(rows)


def _adam_groups(*rows, **kw):
    base = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, decoupled=0, amsgrad=0, maximize=0)
    rows = rows or ({},)
    return (N.AdamGroup * len(rows))(*[N.AdamGroup(**dict(base, **dict(kw, **r))) for r in rows]), len(rows)


def _sgd_groups(*rows, **kw):
    base = dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=0, first_step=1, maximize=0)
    rows = rows or ({},)
    return (N.SgdGroup * len(rows))(*[N.SgdGroup(**dict(base, **dict(kw, **r))) for r in rows]), len(rows)


def test_symbols_and_abi_version():
    lib = N.lib()
    assert lib.osi_abi_version() >= 11
    for name in ("osi_adam_step_groups", "osi_sgd_step_groups"):
        assert hasattr(lib, name) and name in N.declared_symbols()
    header = open(N.CSRC_DIR + "/../../include/osi.h").read()
    for word in ("osi_opt_segment", "osi_adam_group", "osi_sgd_group", "osi_adam_step_groups", "osi_sgd_step_groups"):
        assert word in header
    assert ctypes.sizeof(N.OptSegment) == 12 and ctypes.sizeof(N.AdamGroup) == 64 and ctypes.sizeof(N.SgdGroup) == 48


D = 16   # a dummy non-null "pointer": every case below must be refused before anything is dereferenced on the device


def _adam(n=64, segs=((0, 16, 0),), groups=None, vmax=None, p=D, g=D, m=D, v=D, nseg=None, ngroups=None, seg_ptr=True, grp_ptr=True):
    s, ns = _segs(segs)
    gr, ng = groups if groups is not None else _adam_groups()
    return N.lib().osi_adam_step_groups(p, g, m, v, vmax, n, s if seg_ptr else None, ns if nseg is None else nseg,
                                        gr if grp_ptr else None, ng if ngroups is None else ngroups, 1.0, None)


def _sgd(n=64, segs=((0, 16, 0),), groups=None, p=D, g=D, b=D, nseg=None, ngroups=None, seg_ptr=True, grp_ptr=True):
    s, ns = _segs(segs)
    gr, ng = groups if groups is not None else _sgd_groups()
    return N.lib().osi_sgd_step_groups(p, g, b, n, s if seg_ptr else None, ns if nseg is None else nseg,
                                       gr if grp_ptr else None, ng if ngroups is None else ngroups, 1.0, None)


@pytest.mark.parametrize("call", [_adam, _sgd], ids=["adam", "sgd"])
def test_malformed_tables_are_refused_before_any_launch(call):
    bad = -1
    assert call(p=None) == bad and call(g=None) == bad
    assert call(seg_ptr=False) == bad and call(grp_ptr=False) == bad
    assert call(n=62) == bad and call(n=0) == bad                              # n % 4 != 0
    assert call(nseg=0) == bad and call(ngroups=0) == bad and call(ngroups=17) == bad
    many = tuple((i, i + 1, 0) for i in range(193))
    assert call(n=4 * 200, segs=many) == bad                                    # more than 192 segments
    assert call(segs=((4, 8, 0), (0, 4, 0))) == bad                             # unsorted
    assert call(segs=((0, 8, 0), (7, 12, 0))) == bad                            # overlapping
    assert call(segs=((0, 4, 0), (6, 6, 0))) == bad                             # empty
    assert call(segs=((0, 17, 0),)) == bad                                      # past n / 4
    assert call(segs=((0, 4, 1),)) == bad and call(segs=((0, 4, -1),)) == bad   # group index out of range


def test_group_options_are_refused_before_any_launch():
    assert _adam(m=None) == -1 and _adam(v=None) == -1 and _sgd(b=None) == -1
    assert _adam(groups=_adam_groups(amsgrad=1), vmax=None) == -1               # amsgrad without its arena
    assert _adam(groups=_adam_groups(step=0)) == -1
    assert _adam(segs=((0, 4, 0), (4, 8, 1)), groups=_adam_groups({}, {"step": 0})) == -1
    assert _sgd(groups=_sgd_groups(nesterov=1, momentum=0.0)) == -1
    assert _sgd(groups=_sgd_groups(nesterov=1, dampening=0.5)) == -1


# ---- Python layer ----------------------------------------------------------------------------------------------------------
def _table(opt):
    plain, flat, kgroups = opt._plan_for()
    return plain, [tuple(flat[i:i + 3]) for i in range(0, len(flat), 3)], kgroups


def test_constructions(model):
    head = list(model.logits.parameters())
    body = [p for p in model.parameters() if all(p is not q for q in head)]
    o = optim.SGD([dict(params=head, lr=1e-2), dict(params=body, nesterov=True, weight_decay=5e-4)], lr=1e-3, momentum=0.9)
    assert [g["lr"] for g in o.param_groups] == [1e-2, 1e-3] and [g["nesterov"] for g in o.param_groups] == [False, True]
    assert not _table(o)[0]
    o = optim.AdamW(optim.split_decay(model, 1e-2), lr=1e-3)
    assert [g["weight_decay"] for g in o.param_groups] == [1e-2, 0.0] and all(g["decoupled_weight_decay"] for g in o.param_groups)
    assert all(p.ndim <= 1 for p in o.param_groups[1]["params"]) and all(p.ndim > 1 for p in o.param_groups[0]["params"])
    assert sum(len(g["params"]) for g in o.param_groups) == len(model._plist)
    assert optim.AdamW(model).defaults["weight_decay"] == 1e-2
    o = optim.Adam(head, lr=1e-3)
    assert len(o.param_groups[0]["params"]) == len(head)
    o.add_param_group(dict(params=list(model.resnet_base.fc.parameters()), lr=1e-4, amsgrad=True))
    assert len(o.param_groups) == 2 and o.param_groups[1]["lr"] == 1e-4 and o.param_groups[1]["betas"] == (0.9, 0.999)
    assert len(_table(o)[2]) == 2
    # the reference's spellings still take the plain route
    for legacy in (optim.Adam(model.parameters(), lr=1e-3), optim.Adam(model, lr=1e-3), optim.SGD(params=model.parameters(), lr=0.1)):
        plain, segs, kgroups = _table(legacy)
        assert plain and legacy._plain_options(legacy.param_groups[0]) and len(kgroups) == 1
    assert not optim.Adam(model, weight_decay=1e-4)._plain_options(optim.Adam(model, weight_decay=1e-4).param_groups[0])


def test_refusals(model):
    with pytest.raises(ValueError):                                  # not a view of a model's arena
        optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    with pytest.raises(ValueError):
        optim.SGD(list(model.logits.parameters()) + [torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    other = oi.ResNet50(12, 12, False)
    with pytest.raises(ValueError):                                  # two models
        optim.Adam([dict(params=list(model.logits.parameters())), dict(params=list(other.logits.parameters()))])
    o = optim.Adam(model.logits.parameters())
    with pytest.raises(ValueError):
        o.add_param_group(dict(params=list(other.resnet_base.fc.parameters())))
    assert len(o.param_groups) == 1
    with pytest.raises(ValueError):                                  # one parameter in two groups
        optim.Adam([dict(params=list(model.logits.parameters())), dict(params=list(model.parameters()))])
    # torch's validation of the new arguments
    for make in (lambda: optim.Adam(model, weight_decay=-1.0), lambda: optim.SGD(model, nesterov=True, momentum=0.0),
                 lambda: optim.SGD(model, nesterov=True, dampening=0.1), lambda: optim.SGD(model, weight_decay=-1e-4),
                 lambda: optim.Adam(model, fused=True), lambda: optim.Adam(model, foreach=True), lambda: optim.SGD(model, fused=True),
                 lambda: optim.Adam(model, capturable=True), lambda: optim.AdamW(model, differentiable=True)):
        with pytest.raises(ValueError):
            make()
    optim.Adam(model, foreach=None, fused=False, capturable=False, differentiable=False)


def test_split_decay_table_covers_every_float_once(model):
    o = optim.AdamW(optim.split_decay(model, 1e-2), lr=1e-3)
    plain, segs, kgroups = _table(o)
    assert not plain and [gi for gi, _ in kgroups] == [0, 1] and 2 < len(segs) <= N.OPT_MAX_SEGMENTS
    covered = torch.zeros(model.flat_parameters().numel(), dtype=torch.int32)
    for (b, e, k), nxt in zip(segs, segs[1:] + [None]):
        assert b < e
        if nxt is not None:
            assert e <= nxt[0]                                        # sorted, disjoint
            assert not (e == nxt[0] and k == nxt[2]), "adjacent tensors of one group must merge"
        covered[4 * b:4 * e] += 1
    assert int(covered.max()) == 1
    for (name, off, numel, shape), p in zip(model._pinfo, model._plist):
        assert bool((covered[off:off + numel] == 1).all()), name
    # every unit's group is the group of the tensor it belongs to
    unit_group = torch.full((covered.numel() // 4,), -1, dtype=torch.int32)
    for b, e, k in segs:
        unit_group[b:e] = k
    for (name, off, numel, shape), p in zip(model._pinfo, model._plist):
        want = 0 if p.ndim > 1 else 1
        assert bool((unit_group[off // 4:(off + numel + 3) // 4] == want).all()), name
    # the table is cached until something it depends on changes
    assert o._plan_for()[1] is o._plan_for()[1]
    model._plist[3].requires_grad_(False)                            # a frozen tensor becomes a gap
    try:
        frozen = _table(o)[1]
        off, numel = model._pinfo[3][1], model._pinfo[3][2]
        assert all(e <= off // 4 or b >= (off + numel + 3) // 4 for b, e, k in frozen)
        assert sum(e - b for b, e, k in frozen) == sum(e - b for b, e, k in segs) - ((off + numel + 3) // 4 - off // 4)
    finally:
        model._plist[3].requires_grad_(True)


def test_head_only_table_leaves_the_rest_as_gaps(model):
    o = optim.Adam(model.logits.parameters())
    plain, segs, kgroups = _table(o)
    assert not plain and len(kgroups) == 1
    offs = {id(p): (off, numel) for (name, off, numel, shape), p in zip(model._pinfo, model._plist)}
    want = sorted((offs[id(p)][0] // 4, (offs[id(p)][0] + offs[id(p)][1] + 3) // 4) for p in model.logits.parameters())
    merged = [list(want[0])]
    for b, e in want[1:]:
        if b == merged[-1][1]:
            merged[-1][1] = e
        else:
            merged.append([b, e])
    assert [(b, e) for b, e, k in segs] == [tuple(x) for x in merged]
    assert sum(e - b for b, e, k in segs) * 4 < 0.01 * model.flat_parameters().numel()


def _twin_groups(opt):
    return [dict({k: v for k, v in g.items() if k != "params"}, params=[torch.nn.Parameter(p.detach().clone()) for p in g["params"]])
            for g in opt.param_groups]


def test_state_dict_schema_matches_stock_torch(model):
    head = list(model.logits.parameters())
    body = [p for p in model.parameters() if all(p is not q for q in head)]
    cases = [(optim.AdamW(optim.split_decay(model, 1e-2), lr=1e-3), torch.optim.AdamW),
             (optim.Adam([dict(params=head, amsgrad=True), dict(params=body[:7], weight_decay=1e-3)]), torch.optim.Adam),
             (optim.SGD([dict(params=head, lr=1e-2), dict(params=body, nesterov=True)], lr=1e-3, momentum=0.9), torch.optim.SGD),
             (optim.Adam(model.parameters(), lr=1e-3), torch.optim.Adam),
             (optim.SGD(model, lr=1e-3, momentum=0.9), torch.optim.SGD)]
    for ours, stock in cases:
        twin = stock(_twin_groups(ours))
        a, b = ours.state_dict(), twin.state_dict()
        assert len(a["param_groups"]) == len(b["param_groups"])
        for ga, gb in zip(a["param_groups"], b["param_groups"]):
            assert set(ga) == set(gb) and ga["params"] == gb["params"]
            assert {k: v for k, v in ga.items() if k != "params"} == {k: v for k, v in gb.items() if k != "params"}
        assert a["state"] == {} == b["state"]                       # nothing stepped yet
        twin.load_state_dict(a)
        ours.load_state_dict(b)


def test_legacy_checkpoint_without_the_new_keys_resumes(model):
    """A checkpoint written before the groups carried the new options: the missing keys read as their defaults."""
    for make, drop in ((lambda: optim.Adam(model.parameters(), lr=1e-3), ("decoupled_weight_decay", "weight_decay", "amsgrad", "maximize")),
                       (lambda: optim.SGD(model.parameters(), lr=1e-2, momentum=0.9), ("weight_decay", "dampening", "nesterov", "maximize"))):
        old = make().state_dict()
        for g in old["param_groups"]:
            for k in drop:
                g.pop(k, None)
        fresh = make()
        fresh.load_state_dict(old)
        assert all(k not in fresh.param_groups[0] for k in drop)
        plain, segs, kgroups = _table(fresh)
        assert plain and fresh._plain_options(fresh.param_groups[0])   # and it still takes the plain launch


def test_build_optimizer_reads_the_optional_keys(model):
    from types import SimpleNamespace as NS
    from openset_imagenet.train import build_optimizer
    legacy = build_optimizer(NS(opt=NS(type="adam", lr=1e-3, decay=0, gamma=1)), model)
    assert type(legacy) is optim.Adam and _table(legacy)[0] and legacy._plain_options(legacy.param_groups[0])
    legacy = build_optimizer(NS(opt=NS(type="sgd", lr=1e-2)), model)
    assert type(legacy) is optim.SGD and legacy.param_groups[0]["momentum"] == 0.9 and legacy._plain_options(legacy.param_groups[0])
    o = build_optimizer(NS(opt=NS(type="adamw", lr=1e-3, no_decay="norm_bias", amsgrad=True)), model)
    assert type(o) is optim.AdamW and [g["weight_decay"] for g in o.param_groups] == [1e-2, 0.0] and o.param_groups[0]["amsgrad"]
    o = build_optimizer(NS(opt=NS(type="sgd", lr=1e-2, weight_decay=1e-4, nesterov=True, no_decay="norm_bias")), model)
    assert [g["weight_decay"] for g in o.param_groups] == [1e-4, 0.0] and all(g["nesterov"] for g in o.param_groups)
    o = build_optimizer(NS(opt=NS(type="adam", lr=1e-3, train_only=["logits", "resnet_base.fc"])), model)
    names = {id(p): n for n, p in model.named_parameters()}
    held = sorted(names[id(p)] for g in o.param_groups for p in g["params"])
    assert held == ["logits.weight", "resnet_base.fc.bias", "resnet_base.fc.weight"]
    assert all(p.requires_grad for p in model.parameters())
    with pytest.raises(ValueError):
        build_optimizer(NS(opt=NS(type="adam", lr=1e-3, train_only=["no_such_layer"])), model)


class _NoLaunch:
    """Stands in for torch.ops.osi on a host without a GPU: the bookkeeping around the launch is what these tests look at."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args))


def _step(model, opt, twin, pairs):
    model._grads_fresh = True
    model.bind_gradients()
    for p, t in pairs:
        t.grad = None if p.grad is None else torch.zeros_like(t)
    opt.step()
    twin.step()


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_add_param_group_after_a_step_binds_the_new_state(model, monkeypatch, kind):
    """The added parameters get state entries and their own step count (the kernel steps them), state_dict() lists them like the
    stock optimizer does, and the dict loads both ways."""
    ops = _NoLaunch()
    monkeypatch.setattr(N, "ops", lambda: ops)
    ours, stock = (optim.Adam, torch.optim.Adam) if kind == "adam" else (optim.SGD, torch.optim.SGD)
    extra = dict(lr=3e-4, weight_decay=1e-3, **(dict(amsgrad=True) if kind == "adam" else dict(momentum=0.8)))
    head, added = list(model.logits.parameters()), list(model.resnet_base.fc.parameters())
    pairs = [(p, p.detach().clone().requires_grad_(True)) for p in head + added]
    clone = dict((id(p), t) for p, t in pairs)
    opt = ours(head, lr=1e-3)
    twin = stock([clone[id(p)] for p in head], lr=1e-3, **({} if kind == "adam" else dict(momentum=0.9)))
    _step(model, opt, twin, pairs[:len(head)])
    opt.add_param_group(dict(extra, params=added))
    twin.add_param_group(dict(extra, params=[clone[id(p)] for p in added]))
    assert set(opt.state_dict()["state"]) == set(twin.state_dict()["state"]) == set(range(len(head)))
    _step(model, opt, twin, pairs)
    a, b = opt.state_dict(), twin.state_dict()
    assert [g["params"] for g in a["param_groups"]] == [g["params"] for g in b["param_groups"]]
    assert set(a["state"]) == set(b["state"]) == set(range(len(pairs)))
    for i in b["state"]:
        assert set(a["state"][i]) == set(b["state"][i])
        if kind == "adam":
            assert float(a["state"][i]["step"]) == float(b["state"][i]["step"]) == (2.0 if i < len(head) else 1.0)
    for p in added:                                              # the views are bound into the flat arenas
        st = opt.state[p]
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if kind == "adam" else ("momentum_buffer",):
            assert st[key].untyped_storage().data_ptr() == opt._flat_state[key].untyped_storage().data_ptr()
    assert ops.calls[-1][0] == f"{kind}_step_groups" and len(ops.calls) == 2
    opt2 = ours([dict({k: v for k, v in g.items() if k != "params"}, params=g["params"]) for g in opt.param_groups])
    opt2.load_state_dict(b)
    twin2 = stock([dict({k: v for k, v in g.items() if k != "params"}, params=g["params"]) for g in twin.param_groups])
    twin2.load_state_dict(a)
    if kind == "adam":
        assert [opt2._counts()[opt2._index[id(p)]] for p in head + added] == [2] * len(head) + [1] * len(added)
        assert [float(twin2.state[clone[id(p)]]["step"]) for p in head + added] == [2.0] * len(head) + [1.0] * len(added)
    _step(model, opt2, twin2, pairs)
    assert set(opt2.state_dict()["state"]) == set(twin2.state_dict()["state"])


def test_plain_sgd_without_momentum_keeps_its_first_step_rule_and_its_table(model, monkeypatch):
    """SGD(model, momentum=0) takes the plain launch with first = True on the first step only, and its table is built once."""
    ops = _NoLaunch()
    monkeypatch.setattr(N, "ops", lambda: ops)
    opt = optim.SGD(model, lr=1e-2, momentum=0)
    plans = []
    for _ in range(3):
        model._grads_fresh = True
        opt.step()
        plans.append(opt._plan)
    assert [name for name, _ in ops.calls] == ["sgd_step"] * 3
    assert [args[5] for _, args in ops.calls] == [True, False, False]
    assert plans[1] is not None and plans[2] is plans[1]
    assert opt._steps == 3
    sd = opt.state_dict()
    assert all(v["momentum_buffer"] is None for v in sd["state"].values()) and len(sd["state"]) == len(list(model.parameters()))


def test_build_optimizer_refuses_options_of_the_other_kind(model):
    from types import SimpleNamespace as NS
    from openset_imagenet import train
    with pytest.raises(ValueError, match="amsgrad"):
        train.build_optimizer(NS(opt=NS(type="sgd", lr=1e-3, amsgrad=True)), model)
    with pytest.raises(ValueError, match="nesterov"):
        train.build_optimizer(NS(opt=NS(type="adamw", lr=1e-3, nesterov=True)), model)
    assert isinstance(train.build_optimizer(NS(opt=NS(type="sgd", lr=1e-3, amsgrad=False)), model), optim.SGD)
    legacy = train.build_optimizer(NS(opt=NS(type="adamax", lr=1e-3)), model)     # as before: anything but sgd is Adam
    assert type(legacy) is optim.Adam

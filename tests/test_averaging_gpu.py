"""GPU: weight averaging (EMA / SWA, ABI 20).

1. osi_average_update through torch.ops.osi against torch.lerp on CPU fp32 copies, bit for bit: every weight class, sizes around the
   kernel's tile and grid cap, several spans in one launch, guard bands, the current values untouched, NaN / Inf as torch places them.
2. AveragedModel over a ResNet50: three SGD steps with an update after each against a CPU replay of torch.lerp on the model's arenas;
   the training run itself is bit for bit the run without an average.
3. train(averaged=...) with avg.every and opt.accumulate: the updates follow optimizer steps.
4. ResNet50.bn_momentum: 1.0 leaves the batch statistics, 0.1 restores the default bits.
5. update_bn: the cumulative average of the per-batch statistics.
6. worker(): checkpoints, CSV columns, resume, select: averaged.

Executor tests run the smallest geometry the executor takes: B = 4, 32 x 32 images, fc_layer_dim = out_features = 8.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# csrc/optim.hip: AVG_TILE floats per workgroup tile (256 lanes x one 16-byte unit), AVG_MAX_GRID workgroups at most
T, G = 1024, 2048
GUARD = 64
GUARD_BITS = 0x7FC54321          # a NaN with a payload


def _f32(w):
    return float(torch.tensor(w, dtype=torch.float32))


BELOW_HALF = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))
WEIGHTS = [0.0, _f32(1 - 0.9999), _f32(1 / 3), BELOW_HALF, 0.5, 0.75, 1.0]
SIZES = [4, T - 4, T, T + 4, G * T + 4, 2 * G * T - 4]


def _same(got, ref):
    """torch.equal with NaNs compared as equal"""
    nan = ref.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(ref), ref))


def _guarded(cuda, host):
    """the values on the device with a guard band of GUARD floats behind them: (whole buffer, the view the kernel gets)"""
    n = host.numel()
    whole = torch.empty(n + GUARD, device=cuda)
    whole[:n].copy_(host)
    whole[n:].view(torch.int32).fill_(GUARD_BITS)
    return whole, whole[:n]


def _guard_intact(whole, n):
    return bool((whole[n:].view(torch.int32) == GUARD_BITS).all())


def _run(cuda, pairs, weight):
    """one launch over the (avg, cur) host pairs; returns the averages read back after checking guards and the current values"""
    from openset_imagenet import _native as N
    avg = [_guarded(cuda, a) for a, _ in pairs]
    cur = [c.to(cuda) for _, c in pairs]
    N.ops().average_update([v for _, v in avg], cur, weight)
    torch.cuda.synchronize()
    for (whole, view), c_dev, (_, c) in zip(avg, cur, pairs):
        assert _guard_intact(whole, view.numel()), "the guard band behind an average was written"
        assert torch.equal(c_dev.cpu().view(torch.int32), c.view(torch.int32)), "the current values were written"
    return [view.cpu() for _, view in avg]


@pytest.fixture(scope="module")
def operands():
    gen = torch.Generator().manual_seed(20)
    n = max(SIZES)
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3.0


@pytest.mark.parametrize("n", SIZES)
def test_kernel_bits_against_torch_lerp(cuda, operands, n):
    a, c = operands[0][:n].clone(), operands[1][:n].clone()
    for w in WEIGHTS:
        got, = _run(cuda, [(a, c)], w)
        ref = torch.lerp(a, c, w)
        assert torch.equal(got, ref), f"n={n} weight={w!r}: {int((got != ref).sum())} of {n} elements differ from torch.lerp"
        if w == 1.0:
            assert torch.equal(got.view(torch.int32), c.view(torch.int32))
        if w == 0.0:
            assert torch.equal(got.view(torch.int32), a.view(torch.int32))


@pytest.mark.parametrize("sizes", [(T + 4, 8), (4, 2 * T + 4, T - 4, G * T + 4)])
def test_several_spans_in_one_launch(cuda, operands, sizes):
    pairs, off = [], 0
    for n in sizes:
        pairs.append((operands[0][off:off + n].clone(), operands[1][off:off + n].clone()))
        off += n
    for w in (_f32(1 / 3), 0.75):
        got = _run(cuda, pairs, w)
        for k, ((a, c), g) in enumerate(zip(pairs, got)):
            assert torch.equal(g, torch.lerp(a, c, w)), f"span {k} of {sizes}, weight {w!r}"


def test_nonfinite_values_as_torch_lerp_places_them(cuda, operands):
    n = 3 * T + 4
    a, c = operands[0][:n].clone(), operands[1][:n].clone()
    specials = [float("nan"), float("inf"), float("-inf")]
    for k in range(0, 90):                       # every pairing of {finite, NaN, +Inf, -Inf} in both operands, in several lanes and tiles
        i = 34 * k + 5
        sa, sc = k % 4, (k // 4) % 4
        if sa:
            a[i] = specials[sa - 1]
        if sc:
            c[i] = specials[sc - 1]
    for w in WEIGHTS:
        got, = _run(cuda, [(a, c)], w)
        ref = torch.lerp(a, c, w)
        assert ref.isnan().any() and (ref.isinf().any() or w in (0.0, 1.0))     # (0 * inf: at the end weights every Inf turns NaN)
        assert _same(got, ref), f"weight {w!r}"


def test_ops_refuse_bad_lists(cuda):
    from openset_imagenet import _native as N
    x, y = torch.zeros(8, device=cuda), torch.ones(8, device=cuda)
    for avg, cur, w in (([], [], 0.5), ([x], [y, y], 0.5), ([x], [y[:4]], 0.5), ([x] * 5, [y] * 5, 0.5), ([x], [x], 0.5), ([x], [y], 1.5),
                        ([x], [y], float("nan")), ([x[1:5]], [y[:4]], 0.5)):
        with pytest.raises(RuntimeError):
            N.ops().average_update(avg, cur, w)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.zeros(8))


# ---- 2. the model ------------------------------------------------------------------------------------------------------------------
B, HW, C, STEPS = 4, 32, 8, 3


def _fresh(cuda, seed=7):
    from openset_imagenet import ResNet50
    torch.manual_seed(seed)
    return ResNet50(C, C, False).to(cuda).train()


def _batches(cuda, count, seed=8):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, HW, HW, generator=gen).to(cuda), torch.randint(-1, C, (B,), generator=gen).to(cuda)) for _ in range(count)]


def _arenas(model):
    return (model._flat_params.detach().cpu().clone(), model._flat_buffers.detach().cpu().clone(), model._nbt.cpu().clone(),
            model._flat_grads.detach().cpu().clone())


def _sgd_steps(cuda, averaged_of=None):
    """STEPS SGD steps on the tiny geometry; the arenas before the first and after every step; the AveragedModel when asked for one"""
    from openset_imagenet import EntropicOpensetLoss, optim
    model = _fresh(cuda)
    averaged = averaged_of(model) if averaged_of else None
    opt = optim.SGD(model, lr=0.05, momentum=0.9)
    loss_fn = EntropicOpensetLoss(C, 1.0)
    snaps = [_arenas(model)]
    for x, y in _batches(cuda, STEPS):
        opt.zero_grad()
        logits, _ = model(x)
        loss_fn(logits, y).backward()
        opt.step()
        if averaged is not None:
            averaged.update_parameters(model)
        snaps.append(_arenas(model))
    torch.cuda.synchronize()
    return model, averaged, snaps


@pytest.fixture(scope="module")
def plain_run(cuda):
    """the three steps without an average: the reference every averaged run is compared with, computed once"""
    return _sgd_steps(cuda)[2]


@pytest.mark.parametrize("buffers", ["copy", "average"])
@pytest.mark.parametrize("kind", ["ema", "swa"])
def test_model_average_equals_the_cpu_replay(cuda, plain_run, kind, buffers):
    from openset_imagenet import ResNet50
    from openset_imagenet.averaging import AveragedModel
    model, averaged, snaps = _sgd_steps(cuda, lambda m: AveragedModel(m, kind=kind, decay=0.9, buffers=buffers))
    # the training model did not notice: parameters, buffers, counters and gradients of every step are those of the plain run
    for step, (mine, plain) in enumerate(zip(snaps, plain_run)):
        for name, a, b in zip(("params", "buffers", "nbt", "grads"), mine, plain):
            assert torch.equal(a, b), f"{name} after step {step} differ from the run without an average"
    assert not torch.equal(snaps[0][0], snaps[-1][0])
    # replay: torch.lerp on clones of the model's arenas taken after each step
    avg_p, avg_b = snaps[0][0].clone(), snaps[0][1].clone()
    for n, (p, b, _, _) in enumerate(snaps[1:]):
        w = 1.0 if n == 0 else (1.0 - 0.9 if kind == "ema" else 1.0 / (n + 1))
        w = _f32(w)
        avg_p = torch.lerp(avg_p, p, w)
        avg_b = torch.lerp(avg_b, b, w) if buffers == "average" else b.clone()
    mod = averaged.module
    assert isinstance(mod, ResNet50) and int(averaged.n_averaged) == STEPS
    assert torch.equal(mod._flat_params.cpu(), avg_p), f"{int((mod._flat_params.cpu() != avg_p).sum())} parameters differ from the replay"
    assert torch.equal(mod._flat_buffers.cpu(), avg_b)
    assert torch.equal(mod._nbt.cpu(), model._nbt.cpu()) and int(mod._nbt[0]) == STEPS
    assert not torch.equal(avg_p, snaps[-1][0]), "the average is the model: nothing was averaged"
    # an ordinary model: the same eval-mode logits as a fresh ResNet50 loaded from its state_dict()
    x = _batches(cuda, 1, seed=9)[0][0]
    clone = ResNet50(C, C, False)
    clone.load_state_dict({k: v.cpu() for k, v in mod.state_dict().items()})
    clone = clone.to(cuda).eval()
    mod.eval()
    with torch.no_grad():
        a, b = mod(x)[0], clone(x)[0]
    assert torch.equal(a, b) and bool(a.isfinite().all())


# ---- 3. train() ----------------------------------------------------------------------------------------------------------------------
class Loader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = range(sum(int(y.shape[0]) for _, y in batches))


def _train_once(cuda, opt_block, avg_block):
    """one epoch of train() over 4 batches; the arenas at every update_parameters call with the number of optimizer steps made by then"""
    from openset_imagenet import EntropicOpensetLoss, losses as L, optim, tools
    from openset_imagenet.averaging import AveragedModel, options
    from openset_imagenet.train import train
    from openset_imagenet.util import NameSpace
    tools.set_device_gpu(0)
    model = _fresh(cuda)
    cfg = NameSpace({"parallel": True, "batch_size": B, "loss": {"type": "entropic"}, "opt": dict({"type": "sgd", "lr": 0.05}, **opt_block),
                     "avg": avg_block})
    o = options(cfg)
    averaged = AveragedModel(model, kind=o.kind, decay=o.decay, buffers=o.buffers)
    opt = optim.SGD(model, lr=0.05, momentum=0.9)
    calls, steps = [], [0]
    inner_step, inner_update = opt.step, averaged.update_parameters

    def step(*a, **k):
        steps[0] += 1
        return inner_step(*a, **k)

    def update(m):
        calls.append((steps[0], m._flat_params.detach().cpu().clone()))
        return inner_update(m)
    opt.step, averaged.update_parameters = step, update
    train(model, Loader(_batches(cuda, 4)), opt, EntropicOpensetLoss(C, 1.0), {"j": L.AverageMeter()}, cfg, averaged=averaged)
    torch.cuda.synchronize()
    return model, averaged, calls, steps[0]


def test_train_updates_every_second_optimizer_step(cuda):
    model, averaged, calls, steps = _train_once(cuda, {}, {"kind": "ema", "decay": 0.5, "every": 2})
    assert steps == 4 and [s for s, _ in calls] == [2, 4] and int(averaged.n_averaged) == 2
    replay = torch.lerp(calls[0][1], calls[1][1], 0.5)          # the first update copies, the second averages with 1 - decay
    assert not torch.equal(calls[0][1], calls[1][1])
    assert torch.equal(averaged.module._flat_params.cpu(), replay)
    assert torch.equal(averaged.module._flat_buffers.cpu(), model._flat_buffers.cpu())       # buffers: copy


def test_train_updates_follow_optimizer_steps_under_accumulation(cuda):
    model, averaged, calls, steps = _train_once(cuda, {"accumulate": 2}, {"kind": "ema", "decay": 0.5, "every": 2})
    assert steps == 2 and [s for s, _ in calls] == [2] and int(averaged.n_averaged) == 1          # 4 batches, 2 steps, one update
    assert torch.equal(averaged.module._flat_params.cpu(), model._flat_params.cpu())
    model, averaged, calls, steps = _train_once(cuda, {"accumulate": 3}, {"kind": "ema", "decay": 0.5})   # a ragged last group steps too
    assert steps == 2 and [s for s, _ in calls] == [1, 2]
    assert torch.equal(averaged.module._flat_params.cpu(), torch.lerp(calls[0][1], calls[1][1], 0.5))


def test_train_without_an_average_is_todays_loop(cuda):
    from openset_imagenet import EntropicOpensetLoss, losses as L, optim, tools
    from openset_imagenet.train import train
    from openset_imagenet.util import NameSpace
    tools.set_device_gpu(0)
    cfg = NameSpace({"parallel": True, "batch_size": B, "loss": {"type": "entropic"}, "opt": {"type": "sgd", "lr": 0.05}})
    model = _fresh(cuda)
    trackers = {"j": L.AverageMeter()}
    train(model, Loader(_batches(cuda, 4)), optim.SGD(model, lr=0.05, momentum=0.9), EntropicOpensetLoss(C, 1.0), trackers, cfg)
    with_avg = _train_once(cuda, {}, {"kind": "ema", "decay": 0.5, "every": 2})[0]
    assert list(trackers) == ["j"]
    assert torch.equal(model._flat_params.cpu(), with_avg._flat_params.cpu()) and torch.equal(model._flat_buffers.cpu(), with_avg._flat_buffers.cpu())


# ---- 4. the BatchNorm momentum -------------------------------------------------------------------------------------------------------
def _fresh_buffers(model):
    fresh = torch.zeros(model._flat_buffers.numel())
    for _, bname, arena, off, c in model._binfo:
        if bname == "running_var":
            fresh[off:off + c] = 1.0
    return fresh


def _stat_mask(model):
    """which floats of the buffer arena are statistics (the rest is alignment)"""
    mask = torch.zeros(model._flat_buffers.numel(), dtype=torch.bool)
    for _, bname, arena, off, c in model._binfo:
        if arena == "_flat_buffers":
            mask[off:off + c] = True
    return mask


def _stats_after(model, x, momentum, fresh):
    """the buffer arena after one training-mode forward from fresh buffers under `momentum`"""
    with torch.no_grad():
        model._flat_buffers.copy_(fresh)
        model._nbt.zero_()
        model.bn_momentum = momentum
        model.train()
        model(x)
    torch.cuda.synchronize()
    return model._flat_buffers.cpu().clone()


def test_momentum_one_leaves_the_batch_statistics(cuda):
    model = _fresh(cuda)
    x = _batches(cuda, 1)[0][0]
    r0 = _fresh_buffers(model)
    mask = _stat_mask(model)
    default = _stats_after(model, x, 0.1, r0)
    batch = _stats_after(model, x, 1.0, r0)
    assert model.bn_momentum == 1.0 and int(model._nbt[0]) == 1
    implied = (default.double() - 0.9 * r0.double()) / 0.1                   # solve r = 0.9 r0 + 0.1 b for b
    err = (batch.double() - implied).abs()[mask]
    bound = (2.0 ** -20 * implied.abs().clamp(min=1.0))[mask]
    worst = float((err / bound).max())
    print(f"momentum 1.0: worst |b - implied b| is {worst:.3f} of the bound 2^-20 max(|b|, 1) over {int(mask.sum())} statistics")
    assert bool((err <= bound).all())
    assert float((batch - r0).abs()[mask].max()) > 0.01                       # the statistics moved
    again = _stats_after(model, x, 0.1, r0)
    assert torch.equal(again.view(torch.int32), default.view(torch.int32)), "restoring 0.1 does not reproduce the default forward's buffers"
    # an executor the model creates later (another geometry) starts with the model's value
    model.bn_momentum = 1.0
    x2 = torch.rand(B, 3, 2 * HW, 2 * HW, generator=torch.Generator().manual_seed(3)).to(cuda)
    seen = []
    for m in (None, 1.0, 0.1):                   # None: the executor is created under the value set above
        with torch.no_grad():
            if m is not None:
                model.bn_momentum = m
            model._flat_buffers.copy_(r0)
            model(x2)
        seen.append(model._flat_buffers.cpu().clone())
    assert torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])


# ---- 5. update_bn ----------------------------------------------------------------------------------------------------------------------
def test_update_bn_is_the_cumulative_average(cuda):
    from openset_imagenet import tools
    from openset_imagenet.averaging import AveragedModel, update_bn
    tools.set_device_gpu(0)
    K = 3
    model = _fresh(cuda)
    batches = _batches(cuda, K, seed=11)
    r0 = _fresh_buffers(model)
    mask = _stat_mask(model)
    b = torch.stack([_stats_after(model, x, 1.0, r0).double() for x, _ in batches])      # training-mode statistics do not depend on the buffers
    with torch.no_grad():
        model._flat_buffers.normal_()              # whatever was there is reset
        model._nbt.fill_(40)
    model.bn_momentum = 0.25
    model.eval()
    params = model._flat_params.cpu().clone()
    update_bn(batches, model)
    torch.cuda.synchronize()
    got = model._flat_buffers.cpu().double()
    bound = 8 * K * 2.0 ** -24 * b.abs().max(0).values
    err = (got - b.mean(0)).abs()
    worst = float((err[mask] / bound[mask]).max())
    print(f"update_bn: worst |running - mean_k b_k| is {worst:.3f} of the bound 8 K 2^-24 max_k |b_k| over {int(mask.sum())} statistics")
    assert bool((err[mask] <= bound[mask]).all())
    assert bool((model._nbt == K).all())
    assert model.bn_momentum == 0.25 and not model.training                    # momentum and mode restored
    assert torch.equal(model._flat_params.cpu(), params)                       # parameters untouched
    # plain tensors as batches, through an AveragedModel: the same bits
    averaged = AveragedModel(model)
    with torch.no_grad():
        averaged.module._flat_buffers.zero_()
    update_bn([x for x, _ in batches], averaged)
    assert torch.equal(averaged.module._flat_buffers.cpu().double(), got)
    # restored when the loader fails, too
    def failing():
        yield batches[0]
        raise KeyError("loader")
    model.train()
    with pytest.raises(KeyError):
        update_bn(failing(), model)
    assert model.bn_momentum == 0.25 and model.training
    # frozen statistics would not move
    model.freeze_bn()
    with pytest.raises(ValueError):
        update_bn(batches, model)
    model.freeze_bn(False).freeze_below("layer3")
    with pytest.raises(ValueError):
        update_bn(batches, model)


# ---- 6. worker() -----------------------------------------------------------------------------------------------------------------------
def _cfg(tmp, name, epochs, avg, checkpoint=None):
    from openset_imagenet import util
    cfg = util.load_yaml(os.path.join(os.path.dirname(__file__), "..", "config", "train.yaml"))
    cfg.epochs, cfg.batch_size, cfg.workers, cfg.parallel, cfg.gpu, cfg.protocol = epochs, 8, 0, True, 0, 2
    cfg.loss.type = "entropic"
    cfg.name = name
    cfg.opt.type, cfg.opt.lr, cfg.opt.decay = "adam", 1e-3, 0
    cfg.data.synthetic = 16
    cfg.checkpoint = checkpoint
    cfg.output_directory = str(tmp / name)
    if avg is not None:
        cfg.avg = util.NameSpace(avg)
    return cfg


class _epoch_seeded:
    """worker() shuffles its synthetic loader from torch's global generator, whose state at epoch e depends on everything drawn before:
    a resumed run would see other batches than the straight one. Inside this context every train() call starts from a seed that is a
    function of the epoch alone, so the batches of an epoch are the same in both runs."""

    def __init__(self, first_epoch):
        self.epoch = first_epoch

    def __enter__(self):
        import openset_imagenet.train as T
        self.T, self.inner = T, T.train

        def seeded(*a, **k):
            torch.manual_seed(1000 + self.epoch)
            self.epoch += 1
            return self.inner(*a, **k)
        T.train = seeded

    def __exit__(self, *exc):
        self.T.train = self.inner
        return False


def _final(state):
    m, a = state["model"], state["averaged"]
    return [t.detach().cpu().clone() for t in (m._flat_params, m._flat_buffers, a.module._flat_params, a.module._flat_buffers, a.module._nbt)]


def test_worker_checkpoints_columns_resume_and_selection(cuda, tmp_path):
    import openset_imagenet.train as T
    AVG = {"kind": "ema", "decay": 0.5, "select": "averaged"}
    scores = []
    inner = T.validate

    def spy(model, loader, loss_fn, n_classes, trackers, cfg, shard=None):
        inner(model, loader, loss_fn, n_classes, trackers, cfg, shard=shard)
        scores.append(trackers["conf_kn"].avg + trackers["conf_unk"].avg)
    T.validate = spy
    try:
        with _epoch_seeded(0):
            T.worker(_cfg(tmp_path, "whole", 2, AVG))
    finally:
        T.validate = inner
    whole = _final(T._last_worker_state)
    assert int(T._last_worker_state["averaged"].n_averaged) == 4                 # 2 epochs x 2 steps
    assert list(T._last_worker_state["v_metrics"])[-3:] == ["j_avg", "conf_kn_avg", "conf_unk_avg"]
    assert not torch.equal(whole[0], whole[2])
    ck = torch.load(tmp_path / "whole" / "whole_curr.pth", weights_only=False)
    assert "avg_state_dict" in ck and int(ck["avg_state_dict"]["n_averaged"]) == 4
    assert torch.equal(ck["avg_state_dict"]["module.logits.weight"].cpu(), T._last_worker_state["averaged"].module.logits.weight.detach().cpu())
    rows = open(tmp_path / "whole" / f"scalars-{_cfg(tmp_path, 'whole', 2, AVG).log_name}.csv").read().strip().split("\n")
    assert rows[0] == "epoch,train/loss,val/loss,val/conf_kn,val/conf_unk,val/loss_avg,val/conf_kn_avg,val/conf_unk_avg"
    assert len(rows) == 3 and all(len(r.split(",")) == 8 for r in rows)
    # select: averaged: _best.pth follows the averaged module's score (validate() ran model, averaged, model, averaged)
    assert len(scores) == 4
    model_scores, avg_scores = scores[0::2], scores[1::2]
    assert model_scores != avg_scores
    best = torch.load(tmp_path / "whole" / "whole_best.pth", weights_only=False)
    assert best["best_score"] == max(avg_scores) and ck["best_score"] == avg_scores[-1]
    # resume after one epoch: averaged and trained arenas bit-equal to the straight run
    with _epoch_seeded(0):
        T.worker(_cfg(tmp_path, "part", 1, AVG))
    with _epoch_seeded(1):
        T.worker(_cfg(tmp_path, "resumed", 2, AVG, checkpoint=str(tmp_path / "part" / "part_curr.pth")))
    assert int(T._last_worker_state["averaged"].n_averaged) == 4
    for name, a, b in zip(("params", "buffers", "averaged params", "averaged buffers", "averaged nbt"), _final(T._last_worker_state), whole):
        assert torch.equal(a, b), f"{name} of the resumed run differ from the straight run"


def test_worker_without_the_block_and_with_update_bn(cuda, tmp_path):
    import openset_imagenet.train as T
    T.worker(_cfg(tmp_path, "plain", 1, None))
    assert "averaged" not in T._last_worker_state and list(T._last_worker_state["v_metrics"]) == ["j", "conf_kn", "conf_unk"]
    ck = torch.load(tmp_path / "plain" / "plain_curr.pth", weights_only=False)
    assert sorted(ck) == ["best_score", "epoch", "model_state_dict", "opt_state_dict"]
    head = open(tmp_path / "plain" / f"scalars-{_cfg(tmp_path, 'plain', 1, None).log_name}.csv").readline().strip()
    assert head == "epoch,train/loss,val/loss,val/conf_kn,val/conf_unk"
    # swa from epoch 1 on, statistics re-estimated at the end: {name}_avg.pth
    T.worker(_cfg(tmp_path, "swa", 2, {"kind": "swa", "start_epoch": 1, "update_bn": "on"}))
    averaged = T._last_worker_state["averaged"]
    assert int(averaged.n_averaged) == 2                                          # epoch 0 is not averaged
    ck = torch.load(tmp_path / "swa" / "swa_avg.pth", weights_only=False)
    assert int(ck["avg_state_dict"]["n_averaged"]) == 2 and ck["epoch"] == 2
    assert bool((averaged.module._nbt == 2).all())                                # update_bn over the loader's 2 batches
    assert not torch.equal(averaged.module._flat_buffers.cpu(), T._last_worker_state["model"]._flat_buffers.cpu())

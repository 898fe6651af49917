"""GPU: fine-tuning a suffix (ABI 13). The backward stops at the frozen prefix and a frozen unit gets no weight gradient (derived from
requires_grad alone: same bits as the full run for everything trainable, untouched arena for everything frozen); freeze_below() runs
the prefix in the inference forms (bit-equal to the full frozen run where the launch plans agree, fp64 oracle otherwise and for the
batch-statistics suffix); op counts show the path is shorter; state rules and errors; Adam steps; one worker() run.
Shapes: the project's smallest whole-network cases (B = 4 at 64 x 64, C = 10; B = 3 at 75 x 91, C = 20)."""
import ctypes
import functools
import os

import pytest
import torch

from openset_imagenet import _native as N

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-4        # the project's rel-L2 bar per gradient tensor (tests/test_gate_pinned_gpu.py)
LOGIT_TOL = 1e-4
CUTS = ["layer1.0", "layer2.0", "layer3.2", "layer4.2", "fc"]
MODES = ["train", "freeze_bn", "eval_request"]       # batch statistics | frozen statistics, twice
CONV_DGRAD, CONV_WGRAD, BN_FWD, BN_BWD = 2, 3, 4, 5  # OSI_PROF_* of include/osi.h


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _unit(name):
    from test_finetune_cpu import unit_of_name
    return unit_of_name(name)


def _cut_unit(cut):
    return 17 if cut == "fc" else _unit("resnet_base." + cut + ".conv1.weight")


def _prepare(model, mode):
    """Put the model into one of MODES (the request of eval_request belongs to the next forward only)."""
    model.train(mode != "eval_request").freeze_bn(mode == "freeze_bn")
    if mode == "eval_request":
        model.next_backward()


def _run(model, sd, x, wl, wf, mode, want_x=False, staged=None, poison=True):
    """Reload the state, poison the gradient arena, one forward + loss + backward in `mode`:
    dict(logits, feats, gx, grads, buffers, nbt, arena)."""
    from test_frozen_bn_gpu import _backward
    model.load_state_dict(sd)
    if poison:
        model._flat_grads.fill_(float("nan"))
    model._grad_sync = staged
    try:
        _prepare(model, mode)
        logits, feats, gx, grads = _backward(model, x, wl, wf, want_x=want_x)
    finally:
        model._grad_sync = None
    return dict(logits=logits, feats=feats, gx=gx, grads=grads, buffers=model._flat_buffers.clone(), nbt=model._nbt.clone(),
                arena=model._flat_grads.clone())


@functools.lru_cache(maxsize=None)
def _setup(which):
    """(model, sd, x on the GPU, wl, wf) of one case; the model is shared by the tests of that case, every run reloads `sd`."""
    from test_frozen_bn_gpu import _case, _model
    cuda = torch.device("cuda:0")
    sd, x, wl, wf = _case(which)
    return _model(sd, cuda), sd, x.to(cuda), wl, wf


@functools.lru_cache(maxsize=None)
def _full(which, mode, want_x=False):
    """The full run (every parameter trainable) of one case and mode: computed once, never changed."""
    model, sd, x, wl, wf = _setup(which)
    _set_flags(model, lambda n: True)
    return _run(model, sd, x, wl, wf, mode, want_x=want_x)


def _set_flags(model, trainable):
    model.freeze_below(None)
    for n, p in model.named_parameters():
        p.requires_grad_(bool(trainable(n)))


def _slice_of(model, name):
    for (n, off, numel, _) in model._pinfo:
        if n == name:
            return off, numel
    raise KeyError(name)


def _check_against_full(model, r, full, trainable, frozen_untouched=None):
    """Every trainable tensor's gradient has the bits of the full run; the frozen tensors named by `frozen_untouched` (default: all of
    them) still hold the poison and have no .grad."""
    assert torch.equal(r["logits"], full["logits"]) and torch.equal(r["feats"], full["feats"])
    named = dict(model.named_parameters())
    n_live = 0
    for name in named:
        off, numel = _slice_of(model, name)
        if trainable(name):
            assert name in r["grads"], name
            assert torch.equal(r["grads"][name], full["grads"][name]), f"{name}: not the bits of the full run"
            n_live += 1
        else:
            assert named[name].grad is None and name not in r["grads"], name
            if frozen_untouched is None or frozen_untouched(name):
                assert bool(torch.isnan(r["arena"][off:off + numel]).all()), f"{name}: the frozen slice of the gradient arena was written"
    assert n_live > 0


# ---- 5 / 6: the prefix frozen by hand, both dataflows, one call and stage by stage ---------------------------------------------
@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["signed", "zero_init_residual", "ragged"])
def test_flags_frozen_prefix_same_bits_untouched_arena(cuda, which, mode, cut):
    full = _full(which, mode)
    model, sd, x, wl, wf = _setup(which)
    c = _cut_unit(cut)
    live = lambda n: _unit(n) >= c
    _set_flags(model, live)
    try:
        r = _run(model, sd, x, wl, wf, mode)
    finally:
        _set_flags(model, lambda n: True)
    _check_against_full(model, r, full, live)
    assert len(r["grads"]) == sum(live(n) for n, _ in model.named_parameters()) < len(full["grads"])
    if mode == "train":
        assert torch.equal(r["buffers"], full["buffers"]) and torch.equal(r["nbt"], full["nbt"])
        assert bool((r["nbt"] == sd["resnet_base.bn1.num_batches_tracked"].to(r["nbt"].device) + 1).all())
    else:       # frozen statistics: inputs only
        fresh = {k: v for k, v in sd.items() if "running" in k}
        got = model.state_dict()
        assert all(torch.equal(got[k].cpu(), v) for k, v in fresh.items())


class _Recorder:
    """stand-in for dp's gradient sync at world size 1: the model takes its stage-by-stage path; counts the buckets handed over"""

    def __init__(self):
        self.buckets, self.ranges = 0, []

    def bucket_ready(self, flat, lo, hi, handoff=None):
        self.buckets += 1
        self.ranges.append((lo, hi))

    def finish(self):
        pass


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("mode", ["train", "freeze_bn"])
def test_flags_frozen_prefix_stage_by_stage(cuda, mode, cut):
    which = "signed"
    full = _full(which, mode)
    model, sd, x, wl, wf = _setup(which)
    c = _cut_unit(cut)
    live = lambda n: _unit(n) >= c
    _set_flags(model, live)
    sync = _Recorder()
    try:
        r = _run(model, sd, x, wl, wf, mode, staged=sync)
    finally:
        _set_flags(model, lambda n: True)
    _check_against_full(model, r, full, live)
    stages = model.gradient_buckets()
    holds = [any(live(n) and lo <= off < hi for (n, off, _, _) in model._pinfo) for lo, hi in stages]
    assert sync.buckets == sum(holds) and sync.ranges == [rg for rg, h in zip(stages, holds) if h]
    assert sync.buckets < len(stages) or c <= 3       # a cut above layer1 leaves whole stages without a trainable tensor
    # and the executor is ready for the next step: the last (empty) stage ended the backward
    full_again = _run(model, sd, x, wl, wf, mode, staged=_Recorder())
    for k, g in full["grads"].items():
        assert torch.equal(full_again["grads"][k], g), k


# ---- 7: frozen units in the interior ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "freeze_bn"])
@pytest.mark.parametrize("pattern", ["layer1", "layer3"])
def test_interior_frozen_units(cuda, pattern, mode):
    """layer1 frozen under a trainable stem / layer3 alone frozen: the cut stays at unit 0, the backward runs to full depth, the frozen
    units get no weight gradient."""
    which = "signed"
    full = _full(which, mode)
    model, sd, x, wl, wf = _setup(which)
    live = lambda n: not n.startswith(f"resnet_base.{pattern}.")
    _set_flags(model, live)
    try:
        assert model._trainable_plan()[0] & 1
        r = _run(model, sd, x, wl, wf, mode)
    finally:
        _set_flags(model, lambda n: True)
    _check_against_full(model, r, full, live, frozen_untouched=lambda n: n.endswith("conv1.weight") or n.endswith("conv2.weight")
                        or n.endswith("conv3.weight") or n.endswith("downsample.0.weight"))


# ---- 8: image gradient through a prefix frozen by hand (frozen route) ----------------------------------------------------------------
@pytest.mark.parametrize("cut", ["layer2.0", "fc"])
def test_image_gradient_with_flags_frozen_prefix(cuda, cut):
    which = "signed"
    full = _full(which, "eval_request", True)
    model, sd, x, wl, wf = _setup(which)
    c = _cut_unit(cut)
    live = lambda n: _unit(n) >= c
    _set_flags(model, live)
    try:
        r = _run(model, sd, x, wl, wf, "eval_request", want_x=True)
    finally:
        _set_flags(model, lambda n: True)
    assert r["gx"] is not None and torch.equal(r["gx"], full["gx"]), "x.grad differs from the full run's"
    _check_against_full(model, r, full, live)


# ---- 9: freeze_below on the frozen route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["signed", "ragged"])
def test_freeze_below_frozen_route_same_bits_without_tail_split(cuda, which):
    """Under tail_split = 0 the inference forms and the training topology run the same launch plans: the prefix in the inference forms
    gives the bits of the full frozen run, for the outputs and for every gradient of the suffix."""
    from test_frozen_bn_gpu import _case, _model
    L = N.lib()
    sd, x, wl, wf = _case(which)
    N.check(L.osi_set_tuning(b"tail_split", 0))           # a plan knob: before the executor exists
    try:
        model = _model(sd, cuda)
        xd = x.to(cuda)
        full = _run(model, sd, xd, wl, wf, "freeze_bn")
        for cut in CUTS:
            c = _cut_unit(cut)
            assert model.freeze_below(cut) is model and model.frozen_below == cut
            r = _run(model, sd, xd, wl, wf, "freeze_bn")
            assert model._last[0].trainable == ((0x3FFFF >> c) << c, c)
            _check_against_full(model, r, full, lambda n: _unit(n) >= c)
            assert torch.equal(r["buffers"], full["buffers"]) and torch.equal(r["nbt"], full["nbt"])
        model.freeze_below(None)
        del model
    finally:
        N.check(L.osi_set_tuning(b"tail_split", 1))


def _suffix_gates(model, cut_unit, rec):
    """Gate record for the oracle: the oracle's own recorded decisions (`rec`) for the units below the cut — the executor kept none
    there — and the executor's for the suffix, read through osi_resnet50_debug_gate."""
    import osi_testlib as T
    net, _ = model._last
    lib, dev = N.lib(), model._flat_params.device
    B = next(b for (b, h, w), n in model._nets.items() if n is net)
    relu = []
    C, H, W = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for i in range(lib.osi_resnet50_debug_num_gates(net.h)):
        if (0 if i == 0 else (i - 1) // 3 + 1) < cut_unit:
            relu.append(rec["relu"][i])
            continue
        N.check(lib.osi_resnet50_debug_gate_shape(net.h, i, ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)))
        g = torch.empty(B, C.value, H.value, W.value, dtype=torch.uint8, device=dev)
        N.check(lib.osi_resnet50_debug_gate(net.h, N.ptr(model._ws), i, N.ptr(g), None, T.S()), "debug_gate")
        relu.append(g.cpu().bool())
    return {"relu": relu, "pool_idx": rec["pool_idx"]}


def suffix_oracle(sd, x, wl, wf, dtype, cut_unit, training, gates=None, record=None):
    """One forward + backward of the oracle in `dtype` with the BatchNorms of the units below `cut_unit` in eval mode and the others in
    the mode `training` says: (logits, {key: grad}, the state it ran on). oracle.resnet50_oracle._bn is patched for the call only."""
    from oracle import resnet50_oracle as R
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    leaves = {k: s[k].clone().requires_grad_(True) for k in R.param_keys(s)}
    s.update(leaves)
    orig = R._bn
    R._bn = lambda state, prefix, v, tr: orig(state, prefix, v, bool(tr) and _unit(prefix + ".weight") >= cut_unit)
    try:
        lg, ft = R.forward(s, x.detach().to(dtype), training, gates=gates, record_gates=record)
    finally:
        R._bn = orig
    ((lg * wl.to(dtype)).sum() + (ft * wf.to(dtype)).sum()).backward()
    return lg.detach(), {k: v.grad for k, v in leaves.items()}, s


@functools.lru_cache(maxsize=None)
def _free_record(which, cut_unit, training):
    """The decisions of the free-running fp64 oracle of one case (the prefix part is what the composed gate record takes)."""
    from test_frozen_bn_gpu import _case
    sd, x, wl, wf = _case(which)
    rec = {}
    suffix_oracle(sd, x, wl, wf, torch.float64, cut_unit, training, record=rec)
    return rec


def _judge_suffix(which, cut, training, bar_of):
    """freeze_below(cut) on the GPU against the fp64 oracle under composed gates. bar_of(fp32 CPU oracle's worst error) -> bar."""
    from test_frozen_bn_gpu import _case
    model, sd, x, wl, wf = _setup(which)
    c = _cut_unit(cut)
    _set_flags(model, lambda n: True)
    model.freeze_below(cut)
    try:
        r = _run(model, sd, x, wl, wf, "train" if training else "freeze_bn")
        assert model._last[0].trainable[1] == c
        # train mode records the decisions of the TRAINING forward of the prefix-eval network; frozen: every BatchNorm in eval mode
        rec = _free_record(which, c if training else 0, training)
        gates = _suffix_gates(model, c, rec)
        got_sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    finally:
        model.freeze_below(None)
    cpu = _case(which)
    lg64, g64, _ = suffix_oracle(*cpu, torch.float64, c, training, gates=gates)
    _, g32, s32 = suffix_oracle(*cpu, torch.float32, c, training, gates=gates)
    suffix = [k for k in g64 if _unit(k) >= c]
    assert sorted(r["grads"]) == sorted(suffix)
    live = [k for k in suffix if float(g64[k].abs().max()) > 0]
    cpu_err = max(_rel(g32[k], g64[k]) for k in live)
    bar = bar_of(cpu_err)
    errs = {k: _rel(r["grads"][k].cpu(), g64[k]) for k in live}
    worst = max(errs, key=errs.get)
    lerr = float((r["logits"].cpu().double() - lg64).abs().max())
    print(f"freeze_below({cut}) {which} {'batch' if training else 'frozen'} statistics: worst tensor {errs[worst]:.2e} ({worst}), "
          f"median {sorted(errs.values())[len(errs) // 2]:.2e}, logits {lerr:.2e}; fp32 CPU oracle worst {cpu_err:.2e}, bar {bar:.2e}; "
          f"{len(suffix) - len(live)} suffix tensors exactly zero")
    for k in suffix:
        if k not in live:
            assert float(r["grads"][k].abs().max()) == 0.0, f"{k}: the reference is exactly zero"
    for k, e in errs.items():
        assert e <= bar, f"{k}: rel-L2 {e:.2e} > {bar:.2e}"
    assert lerr <= LOGIT_TOL * max(1.0, float(lg64.abs().max())) if not training else lerr <= LOGIT_TOL
    return c, sd, got_sd, s32


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("which", ["signed", "zero_init_residual", "ragged"])
def test_freeze_below_frozen_route_vs_fp64_oracle(cuda, which, cut):
    """At the default launch plans. Bar: the existing frozen test's, min(10 x the fp32 CPU oracle's worst error in this case, 5e-4)."""
    c, sd, got, _ = _judge_suffix(which, cut, False, lambda cpu_err: min(10 * cpu_err, GRAD_TOL))
    for k, v in sd.items():
        if "running" in k or "tracked" in k:
            assert torch.equal(got[k], v), f"{k}: a frozen-statistics step wrote it"


BATCH_CASES = ([("ragged", c) for c in ("layer2.0", "layer3.2", "layer4.2", "fc")] + [("zero_init_residual", c) for c in CUTS] +
               [("signed", c) for c in ("layer1.0", "layer4.2", "fc")])


@pytest.mark.parametrize("which,cut", BATCH_CASES)
def test_freeze_below_batch_statistics_suffix_vs_fp64_oracle(cuda, which, cut):
    """Bar: GRAD_TOL per live suffix tensor, LOGIT_TOL. The fp32 CPU oracle's own worst error under the same gates has to be within a
    third of the bar before the GPU is judged (the headroom tests/test_gate_pinned_gpu.py documents); the cases where it is not
    (signed at layer2.0 / layer3.2, ragged at layer1.0: 1.8e-4 - 2.5e-4) are not in the list."""
    def bar_of(cpu_err):
        assert cpu_err <= GRAD_TOL / 3, f"the fp32 CPU oracle itself is {cpu_err:.2e} from fp64: the case does not carry the bar"
        return GRAD_TOL
    c, sd, got, s32 = _judge_suffix(which, cut, True, bar_of)
    moved = 0
    for k, v in sd.items():
        if not ("running" in k or "tracked" in k):
            continue
        if _unit(k) < c:
            assert torch.equal(got[k], v), f"{k}: statistics of the frozen prefix changed"
        elif k.endswith("tracked"):
            assert int(got[k]) == int(v) + 1, k
        else:
            assert not torch.equal(got[k], v), f"{k}: the suffix ran on batch statistics and did not update it"
            assert torch.allclose(got[k], s32[k].float(), rtol=1e-3, atol=1e-5), k
            moved += 1
    assert moved == 2 * sum(1 for k in sd if k.endswith("running_mean") and _unit(k) >= c)


# ---- 11: the path really is shorter ------------------------------------------------------------------------------------------------
def _op_counts(model, x, wl, wf, mode):
    """(forward op counts, backward op counts) per OSI_PROF class of one step in `mode` (executor profile mode 1)."""
    from test_frozen_bn_gpu import _loss
    L = N.lib()
    net = model._last[0]
    ms, cnt = (ctypes.c_double * 7)(), (ctypes.c_int * 7)()
    N.check(L.osi_resnet50_profile(net.h, 1))
    try:
        for p in model.parameters():
            p.grad = None
        _prepare(model, mode)
        logits, feats = model(x)
        assert model._last[0] is net
        N.check(L.osi_resnet50_profile_read(net.h, ms, cnt))
        fwd = list(cnt)
        _loss(logits, feats, wl.to(x.device), wf.to(x.device)).backward()
        N.check(L.osi_resnet50_profile_read(net.h, ms, cnt))
        bwd = list(cnt)
    finally:
        N.check(L.osi_resnet50_profile(net.h, 0))
    torch.cuda.synchronize()
    return fwd, bwd


def test_op_counts_show_the_shorter_path(cuda):
    model, sd, x, wl, wf = _setup("signed")
    _set_flags(model, lambda n: True)
    _run(model, sd, x, wl, wf, "train")                  # the executor of this geometry exists
    counts = {}
    for mode in ("train", "freeze_bn"):
        model.load_state_dict(sd)
        counts[mode, "full"] = _op_counts(model, x, wl, wf, mode)
        for cut in ("layer4.0", "fc"):
            c = _cut_unit(cut)
            _set_flags(model, lambda n: _unit(n) >= c)
            counts[mode, cut] = _op_counts(model, x, wl, wf, mode)
            _set_flags(model, lambda n: True)
    model.freeze_below("fc")
    counts["freeze_bn", "below fc"] = _op_counts(model, x, wl, wf, "freeze_bn")
    counts["train", "below fc"] = _op_counts(model, x, wl, wf, "train")
    model.freeze_below(None)
    model.load_state_dict(sd)
    for k, (f, b) in counts.items():
        print(k, "forward", f, "backward", b)
    for mode in ("train", "freeze_bn"):
        full_f, full_b = counts[mode, "full"]
        assert min(full_b[CONV_DGRAD], full_b[CONV_WGRAD], full_b[BN_BWD]) > 0
        f, b = counts[mode, "fc"]
        assert (b[CONV_DGRAD], b[CONV_WGRAD], b[BN_BWD]) == (0, 0, 0), "head-only fine-tuning still differentiates the backbone"
        assert f == full_f                               # flags alone do not change the forward
        f, b = counts[mode, "layer4.0"]
        for cls in (CONV_DGRAD, CONV_WGRAD, BN_BWD):
            assert 0 < b[cls] < full_b[cls], (mode, cls, b[cls], full_b[cls])
        f, b = counts[mode, "below fc"]
        assert (b[CONV_DGRAD], b[CONV_WGRAD], b[BN_BWD]) == (0, 0, 0)
        assert f[BN_FWD] < full_f[BN_FWD], "the prefix still runs the training topology's BatchNorm passes"


# ---- 12: state and errors ------------------------------------------------------------------------------------------------------------
def test_state_and_errors(cuda):
    from test_frozen_bn_gpu import _loss
    model, sd, x, wl, wf = _setup("signed")
    L = N.lib()
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    full_gx = _full("signed", "eval_request", True)["gx"]
    _set_flags(model, lambda n: True)
    model.load_state_dict(sd)
    model.freeze_below("layer3.2")
    c = _cut_unit("layer3.2")
    try:
        model.train().freeze_bn()
        logits, feats = model(x)
        net = model._last[0]
        mask, p = ctypes.c_uint(), ctypes.c_int()
        assert L.osi_resnet50_get_trainable(net.h, ctypes.byref(mask), ctypes.byref(p)) == 0
        assert (mask.value, p.value) == ((0x3FFFF >> c) << c, c)
        # the setting holds for the forward and its backward
        assert L.osi_resnet50_set_trainable(net.h, 0x3FFFF, 0) == -3
        # the gates of the prefix do not exist; a suffix gate reads
        C, H, W = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        N.check(L.osi_resnet50_debug_gate_shape(net.h, 3 * c, ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)))
        g = torch.empty(x.shape[0], C.value, H.value, W.value, dtype=torch.uint8, device=cuda)
        am = torch.empty(x.shape[0], 64, 16, 16, dtype=torch.int32, device=cuda)
        assert L.osi_resnet50_debug_gate(net.h, N.ptr(model._ws), 0, N.ptr(g), N.ptr(am), st()) == -3
        for i in (1, 3 * (c - 1), 3 * (c - 1) - 1):       # first block's bn1, the block output and bn2 of the last prefix block
            assert L.osi_resnet50_debug_gate(net.h, N.ptr(model._ws), i, N.ptr(g), None, st()) == -3, i
        assert L.osi_resnet50_debug_gate(net.h, N.ptr(model._ws), 3 * c, N.ptr(g), None, st()) == 0
        assert L.osi_resnet50_debug_gate(net.h, N.ptr(model._ws), 3 * (c - 1) + 1, N.ptr(g), None, st()) == 0
        # no image gradient behind an inference-form prefix: refused, nothing launched, and the backward can still be finished
        wl_d, wf_d = wl.to(cuda).contiguous(), wf.to(cuda).contiguous()
        dimg = torch.full_like(x, float("nan"))
        xadv = torch.empty(x.shape[0], x.shape[2], x.shape[3], 4, device=cuda)
        args = lambda dimage, s: (net.h, N.ptr(model._flat_params), N.ptr(model._flat_grads), N.ptr(model._ws), N.ptr(wl_d), N.ptr(wf_d),
                                  N.ptr(dimage), 1, s, s + 1, st())
        assert L.osi_resnet50_backward_ex(*args(dimg, 0)) == -3
        assert L.osi_resnet50_backward_adv(net.h, N.ptr(model._flat_params), N.ptr(model._flat_grads), N.ptr(model._ws), N.ptr(wl_d),
                                           N.ptr(wf_d), N.ptr(xadv), 0.1, 0.0, 1.0, 0, 4, st()) == -3
        with pytest.raises(RuntimeError, match="BEFORE the forward"):
            model.next_backward(fgsm=0.01)
        assert model._bw_request is None
        model._flat_grads.fill_(float("nan"))
        for s in range(model._n_stages):
            assert L.osi_resnet50_backward_ex(*args(None, s)) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(dimg).all())
        off, numel = _slice_of(model, "resnet_base.layer4.1.conv2.weight")
        assert bool(torch.isfinite(model._flat_grads[off:off + numel]).all())
        off, numel = _slice_of(model, "resnet_base.layer3.1.conv2.weight")
        assert bool(torch.isnan(model._flat_grads[off:off + numel]).all())
        assert L.osi_resnet50_set_trainable(net.h, (0x3FFFF >> c) << c, c) == 0       # the backward is over: accepted again
        # an abandoned forward does not block the next step's setting
        model(x)
        model.freeze_below("layer4")
        lg, ft = model(x)
        _loss(lg, ft, wl_d, wf_d).backward()
        model.freeze_below("layer3.2")

        # image gradients through the declared prefix: batch-statistics suffix refuses, the frozen route keeps the full topology
        model.freeze_bn(False).train()
        with pytest.raises(RuntimeError, match="freeze_bn"):
            model(x.clone().requires_grad_())
        model.next_backward(fgsm=0.01)
        with pytest.raises(RuntimeError, match="freeze_bn"):
            model(x)
        model._bw_request = None
        model.eval()
        xi = x.clone().requires_grad_()
        lg, ft = model(xi)
        assert model._last[0].trainable[1] == 0
        _loss(lg, ft, wl_d, wf_d).backward()
        torch.cuda.synchronize()
        assert xi.grad is not None and bool(torch.isfinite(xi.grad).all()) and float(xi.grad.abs().max()) > 0
        assert torch.equal(xi.grad, full_gx)

        # a prefix parameter re-enabled by hand contradicts the declaration
        model.train()
        name = "resnet_base.layer2.1.bn2.weight"
        dict(model.named_parameters())[name].requires_grad_(True)
        with pytest.raises(RuntimeError, match=name.replace(".", r"\.")):
            model(x)
        dict(model.named_parameters())[name].requires_grad_(False)
        model(x)
    finally:
        model._bw_request = None
        model.freeze_below(None)
        model.freeze_bn(False)
        _set_flags(model, lambda n: True)
        model.load_state_dict(sd)


# ---- 13: optimizer steps -------------------------------------------------------------------------------------------------------------
def test_three_adam_steps_below_layer4(cuda):
    from openset_imagenet import optim
    from test_frozen_bn_gpu import _backward, _case, _model
    sd, x, wl, wf = _case("signed")
    xd = x.to(cuda)
    model = _model(sd, cuda).train()
    opt = optim.Adam(model.parameters(), lr=1e-3)
    assert model.freeze_below("layer4") is model
    c = _cut_unit("layer4.0")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for step in range(3):
        if step == 2:
            with torch.no_grad():                         # validate() between two steps
                model.eval()
                model(xd)
                model.train()
        opt.zero_grad()
        logits, feats = model(xd)
        loss = (logits * wl.to(cuda)).sum() + (feats * wf.to(cuda)).sum()
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss)), step
    torch.cuda.synchronize()
    after = model.state_dict()
    for k, v in before.items():
        if _unit(k) < c:
            assert torch.equal(after[k], v), f"{k}: the frozen prefix changed"
        elif k.endswith("tracked"):
            assert int(after[k]) == int(v) + 3, k
        else:
            assert not torch.equal(after[k], v), f"{k}: the suffix did not move"
    # released: a step is the one of a model that never declared a cut
    model.load_state_dict(sd)
    assert model.freeze_below(None) is model and model.frozen_below is None and all(p.requires_grad for p in model.parameters())
    fresh = _model(sd, cuda).train()
    a = _backward(model, xd, wl, wf, want_x=False)
    b = _backward(fresh, xd, wl, wf, want_x=False)
    assert torch.equal(a[0], b[0]) and a[3].keys() == b[3].keys() and len(a[3]) == 162
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    for m in (model, fresh):
        optim.Adam(m.parameters(), lr=1e-3).step()
    torch.cuda.synchronize()
    assert torch.equal(model._flat_params, fresh._flat_params) and torch.equal(model._flat_buffers, fresh._flat_buffers)
    assert torch.equal(model._nbt, fresh._nbt)


# ---- 14: the training loop ---------------------------------------------------------------------------------------------------------
def _cfg(tmp, name, epochs, checkpoint=None, **extra):
    from openset_imagenet import util
    cfg = util.load_yaml(os.path.join(os.path.dirname(__file__), "..", "config", "train.yaml"))
    cfg.epochs, cfg.batch_size, cfg.workers, cfg.parallel, cfg.gpu, cfg.protocol = epochs, 8, 0, True, 0, 2
    cfg.loss.type = "entropic"
    cfg.name = name
    cfg.opt.type, cfg.opt.lr = "adam", 1e-3
    cfg.data.synthetic = 16
    cfg.checkpoint = checkpoint
    cfg.output_directory = str(tmp / name)
    for k, v in extra.items():
        setattr(cfg, k, v)
    return cfg


def test_worker_with_freeze_below(cuda, tmp_path):
    from openset_imagenet.train import worker, _last_worker_state
    worker(_cfg(tmp_path, "base", 1))
    base = tmp_path / "base" / "base_curr.pth"
    worker(_cfg(tmp_path, "tuned", 2, checkpoint=str(base), train_mode="finetune", freeze_below="layer4"))
    assert _last_worker_state["model"].frozen_below == "layer4.0"
    tuned = tmp_path / "tuned" / "tuned_curr.pth"
    assert tuned.is_file()
    s0 = torch.load(base, weights_only=False)["model_state_dict"]
    s1 = torch.load(tuned, weights_only=False)["model_state_dict"]
    c = _cut_unit("layer4.0")
    moved = 0
    for k, v in s0.items():
        if _unit(k) < c:
            assert torch.equal(s1[k].cpu(), v.cpu()), f"{k}: the frozen prefix changed"
        elif not k.endswith("tracked"):
            moved += int(not torch.equal(s1[k].cpu(), v.cpu()))
    assert moved > 0

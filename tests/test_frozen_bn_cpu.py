"""CPU: the frozen-statistics BatchNorm backward (ABI 12) — symbols, argument validation without a GPU, the executor's state rule,
and the anchor of the GPU bar: how far the torch-CPU fp32 oracle in EVAL mode is from fp64 under its own gates."""
import ctypes
import os
import re

import pytest
import torch

from openset_imagenet import _native as N
from oracle import resnet50_oracle as R

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("osi_bn_frozen_coeffs_multi", "osi_conv_dgrad_fused_frozen", "osi_bn_backward_frozen", "osi_bn_relu_maxpool_bwd_frozen",
       "osi_resnet50_forward_frozen")
ERR_ARG, ERR_STATE = -1, -3


def test_frozen_symbols_declared_exported_and_bound():
    lib = N.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "osi.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in include/osi.h"
        assert hasattr(lib, s), f"{s} is not exported by libosi_hip.so"
        assert s in N.declared_symbols(), f"{s} is missing from the ctypes table"
    assert lib.osi_abi_version() >= 12
    # the ctypes mirrors have the sizes of the C structs (8 / 7 pointers, padded int)
    assert ctypes.sizeof(N.BnFrozenLayer) == 72 and ctypes.sizeof(N.BnFrozenConsumer) == 56


def test_frozen_entries_refuse_bad_arguments_without_launching():
    """OSI_ERR_ARG before any launch: safe on a host without a GPU (a launch there would be OSI_ERR_LAUNCH)."""
    lib = N.lib()
    p = 4096                      # a non-NULL "pointer" that is never dereferenced: every call below fails its preconditions first
    assert lib.osi_bn_frozen_coeffs_multi(None, 1, 1e-5, None) == ERR_ARG
    tab = (N.BnFrozenLayer * 2)()
    tab[0] = N.BnFrozenLayer(p, p, p, p, p, p, p, p, 64)
    tab[1] = N.BnFrozenLayer(p, p, p, p, p, p, p, None, 64)           # invstd missing
    assert lib.osi_bn_frozen_coeffs_multi(tab, 2, 1e-5, None) == ERR_ARG
    assert lib.osi_bn_frozen_coeffs_multi(tab, 0, 1e-5, None) == ERR_ARG
    assert lib.osi_bn_frozen_coeffs_multi(tab, 55, 1e-5, None) == ERR_ARG

    from osi_testlib import Fusion
    d = N.ConvDesc.make(2, 8, 8, 64, 64, 1, 1, 0)
    P = ctypes.c_int(-7)
    dg = lib.osi_conv_dgrad_fused_frozen
    assert dg(ctypes.byref(d), p, p, p, None, 0, ctypes.byref(P), None) == ERR_ARG                      # no fusion block
    f = Fusion(y0=p, scale0=p, shift0=None)
    assert dg(ctypes.byref(d), p, p, p, ctypes.byref(f), 0, ctypes.byref(P), None) == ERR_ARG          # gate needs scale0 AND shift0
    f = Fusion(y0=p, scale0=p, shift0=p, relu_mask=p)
    assert dg(ctypes.byref(d), p, p, p, ctypes.byref(f), 0, ctypes.byref(P), None) == ERR_ARG          # a bitmask is the block-input form
    f = Fusion(y0=p, scale0=p, shift0=p, y1=p, mean1=p, invstd1=p)
    assert dg(ctypes.byref(d), p, p, p, ctypes.byref(f), 0, ctypes.byref(P), None) == ERR_ARG          # one consumer only
    f = Fusion(y0=p, scale0=p, shift0=p)
    assert dg(ctypes.byref(d), p, p, p, ctypes.byref(f), N.TILE_128x128, ctypes.byref(P), None) == ERR_ARG   # 64x64 forms only
    assert dg(ctypes.byref(d), None, p, p, ctypes.byref(f), 0, ctypes.byref(P), None) == ERR_ARG
    f = Fusion(y0=p, scale0=p, shift0=p, partials=p, partials_bytes=1 << 20)                           # sums need mean0 / invstd0
    assert dg(ctypes.byref(d), p, p, p, ctypes.byref(f), 0, ctypes.byref(P), None) == ERR_ARG
    assert P.value == -7

    bw = lib.osi_bn_backward_frozen
    c = (N.BnFrozenConsumer * 2)()
    c[0] = N.BnFrozenConsumer(p, p, p, p, p, None, None)
    assert bw(None, None, c, 1, None, 297, 64, None, 0, None) == ERR_ARG
    assert bw(p, None, None, 1, None, 297, 64, None, 0, None) == ERR_ARG
    assert bw(p, None, c, 3, None, 297, 64, None, 0, None) == ERR_ARG
    assert bw(p, None, c, 1, None, 297, 66, None, 0, None) == ERR_ARG                                   # C % 4
    c[0] = N.BnFrozenConsumer(p, p, p, p, p, p, None)                                                   # dgamma without dbeta
    assert bw(p, None, c, 1, None, 297, 64, p, 1 << 20, None) == ERR_ARG
    c[0] = N.BnFrozenConsumer(p, p, p, p, p, p, p)                                                      # reductions without a workspace
    assert bw(p, None, c, 1, None, 297, 64, None, 0, None) == ERR_ARG
    c[0] = N.BnFrozenConsumer(p, p, p, p, p, None, None)
    c[1] = N.BnFrozenConsumer(p, p, p, p, p, None, None)                                                # both consumers into one buffer
    assert bw(p, None, c, 2, None, 297, 64, None, 0, None) == ERR_ARG

    st = lib.osi_bn_relu_maxpool_bwd_frozen
    assert st(p, None, p, p, p, p, p, None, None, 2, 16, 16, 64, None, 0, None) == ERR_ARG              # no arg-max bytes
    assert st(p, p, p, p, p, None, p, None, None, 2, 16, 16, 64, None, 0, None) == ERR_ARG              # no scale
    assert st(p, p, p, p, p, p, p, p, p, 2, 16, 16, 64, None, 0, None) == ERR_ARG                       # reductions without a workspace


def test_executor_state_rule_without_gpu():
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(h), 2, 64, 64, 10, 10, 0) == 0
    try:
        p = 4096
        assert lib.osi_resnet50_forward_frozen(h, None, p, p, p, p, p, None) == ERR_ARG
        assert lib.osi_resnet50_forward_frozen(h, p, None, p, p, p, p, None) == ERR_ARG
        assert lib.osi_resnet50_forward_frozen(h, p, p, p, None, p, p, None) == ERR_ARG
        assert lib.osi_resnet50_forward_frozen(None, p, p, p, p, p, p, None) == ERR_ARG
        # a backward without a forward (of either kind) is still refused, not launched
        assert lib.osi_resnet50_backward(h, p, p, p, p, None, 0, 1, None) == ERR_STATE
        assert lib.osi_resnet50_backward_ex(h, p, None, p, p, None, p, 0, 0, 4, None) == ERR_STATE
    finally:
        lib.osi_resnet50_destroy(h)


def test_freeze_bn_flag_and_config_key():
    from openset_imagenet import ResNet50
    from openset_imagenet import train as T
    m = ResNet50(10, 10, False)
    assert m.bn_frozen is False and m.training
    assert m.freeze_bn() is m and m.bn_frozen is True and m.training          # model.training keeps its meaning
    assert m.freeze_bn(False) is m and m.bn_frozen is False
    with pytest.raises(AttributeError):
        m.bn_frozen = True

    class Cfg:
        pass
    cfg = Cfg()
    assert T._freeze_bn_of(cfg) is False                                      # absent = off
    for value, want in ((True, True), (False, False), ("on", True), ("off", False)):
        cfg.freeze_bn = value
        assert T._freeze_bn_of(cfg) is want
    cfg.freeze_bn = "maybe"
    with pytest.raises(ValueError):
        T._freeze_bn_of(cfg)


# ---- the anchor of the GPU bar ---------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def eval_oracle(sd, x, wl, wf, dtype, gates=None, record=None):
    """One eval-mode forward + backward of the oracle in `dtype`: (logits, x.grad, {key: grad}, the state it ran on)."""
    s = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    leaves = {k: s[k].clone().requires_grad_(True) for k in R.param_keys(s)}
    s.update(leaves)
    xi = x.detach().to(dtype).clone().requires_grad_()
    lg, ft = R.forward(s, xi, False, gates=gates, record_gates=record)
    ((lg * wl.to(dtype)).sum() + (ft * wf.to(dtype)).sum()).backward()
    return lg.detach(), xi.grad, {k: v.grad for k, v in leaves.items()}, s


def anchor_case(which):
    """(sd, x, wl, wf): B = 4 at 64 x 64 on the signed BatchNorm state, or B = 3 at 75 x 91 (positive state, C = 20)."""
    if which == "signed":
        from osi_testlib import NET_B, NET_C, network_case
        sd, x, _ = network_case("signed")
        B, C, seed = NET_B, NET_C, 101
    else:
        B, C, seed = 3, 20, 7
        gen = torch.Generator().manual_seed(seed)
        sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), generator=gen)
        x = torch.rand(B, 3, 75, 91, generator=gen)
    gen = torch.Generator().manual_seed(seed + 1)
    return sd, x, torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen) * 0.1


@pytest.mark.parametrize("which", ["signed", "ragged"])
def test_eval_mode_fp32_oracle_is_within_1e5_of_fp64_under_its_own_gates(which):
    """With frozen statistics nothing couples the rows of a batch, so fp32 sits two orders of magnitude closer to fp64 than in training
    mode (1.3e-4): measured 2.7e-6 worst tensor. This is what the GPU test's bar (10 x the fp32 oracle's own error) stands on."""
    sd, x, wl, wf = anchor_case(which)
    rec = {}
    lg32, gx32, g32, s32 = eval_oracle(sd, x, wl, wf, torch.float32, record=rec)
    lg64, gx64, g64, _ = eval_oracle(sd, x, wl, wf, torch.float64, gates=rec)
    assert len(g32) == 162
    errs = {k: _rel(g32[k], g64[k]) for k in g32 if float(g64[k].abs().max()) > 0}
    for k in g32:
        if k not in errs:
            assert float(g32[k].abs().max()) == 0.0, f"{k}: fp64 gradient exactly zero, fp32 not"
    worst = max(errs, key=errs.get)
    print(f"{which}: x.grad {_rel(gx32, gx64):.2e}, worst tensor {errs[worst]:.2e} ({worst}), "
          f"median {sorted(errs.values())[len(errs) // 2]:.2e}")
    assert _rel(gx32, gx64) <= 1e-5
    assert errs[worst] <= 1e-5, worst
    for k in sd:                                # eval mode: the running statistics and the batch counters are inputs only
        if "running" in k or "tracked" in k:
            assert torch.equal(s32[k], sd[k]), k

"""Helpers for the GPU parity tests: every call goes through the C ABI of libosi_hip.so (ctypes), torch is only the allocator."""
import ctypes

import torch

from openset_imagenet import _native as N


def S():
    return torch.cuda.current_stream().cuda_stream


class pinned_knobs:
    """`with pinned_knobs(bn_grid=7, ...)`: sets the tuning knobs on entry and restores what they were on exit."""

    def __init__(self, **settings):
        self.settings, self.prev = settings, []

    def __enter__(self):
        lib = N.lib()
        for k in self.settings:
            v = ctypes.c_int()
            N.check(lib.osi_get_tuning(k.encode(), ctypes.byref(v)), k)
            self.prev.append((k, v.value))
        try:
            for k, v in self.settings.items():
                N.check(lib.osi_set_tuning(k.encode(), v), f"{k} = {v}")
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            N.check(N.lib().osi_set_tuning(k.encode(), v), k)
        return False


def nhwc(x):          # NCHW tensor -> contiguous NHWC copy
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):          # NHWC tensor -> NCHW view
    return x.permute(0, 3, 1, 2)


def krsc(w):          # OIHW -> [O][R][S][I]
    return w.permute(0, 2, 3, 1).contiguous()


def oihw(w):
    return w.permute(0, 3, 1, 2)


def conv_fwd(x_nhwc, w_krsc, k, stride, pad, tile=0, y=None):
    """y: the caller's output buffer (default: a fresh one)."""
    B, H, W, Cin = x_nhwc.shape
    Cout = w_krsc.shape[0]
    d = N.ConvDesc.make(B, H, W, Cin, Cout, k, stride, pad)
    if y is None:
        y = torch.empty(B, d.Ho, d.Wo, Cout, device=x_nhwc.device)
    N.check(N.lib().osi_conv_fwd(ctypes.byref(d), N.ptr(x_nhwc), N.ptr(w_krsc), N.ptr(y), tile, S()), "conv_fwd")
    return y


def conv_dgrad(dy_nhwc, w_krsc, H, W, k, stride, pad, accumulate_into=None, tile=0, accumulate=None):
    """accumulate_into: the caller's buffer; accumulate: the mode it is passed with (default: 1 when a buffer is given, else 0)."""
    B, Ho, Wo, Cout = dy_nhwc.shape
    Cin = w_krsc.shape[3]
    d = N.ConvDesc.make(B, H, W, Cin, Cout, k, stride, pad)
    assert (d.Ho, d.Wo) == (Ho, Wo)
    dx = accumulate_into if accumulate_into is not None else torch.full((B, H, W, Cin), float("nan"), device=dy_nhwc.device)
    N.check(N.lib().osi_conv_dgrad(ctypes.byref(d), N.ptr(dy_nhwc), N.ptr(w_krsc), N.ptr(dx), int(accumulate_into is not None) if accumulate is None else accumulate, tile, S()),
            "conv_dgrad")
    return dx


def conv_wgrad(dy_nhwc, x_nhwc, k, stride, pad, dw=None, ws=None):
    """dw / ws: the caller's output and workspace (ws: uint8, exactly osi_conv_wgrad_workspace(d) bytes; default: fresh ones)."""
    B, H, W, Cin = x_nhwc.shape
    Cout = dy_nhwc.shape[3]
    d = N.ConvDesc.make(B, H, W, Cin, Cout, k, stride, pad)
    stem = Cin == 4 and k == 7
    ktot = 224 if stem else k * k * Cin
    if dw is None:
        dw = torch.full((Cout, ktot), float("nan"), device=x_nhwc.device)
    nbytes = N.lib().osi_conv_wgrad_workspace(ctypes.byref(d))
    if ws is None:
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x_nhwc.device)
    else:
        assert ws.numel() == nbytes
    N.check(N.lib().osi_conv_wgrad(ctypes.byref(d), N.ptr(dy_nhwc), N.ptr(x_nhwc), N.ptr(dw), N.ptr(ws) if nbytes else None, nbytes, S()), "conv_wgrad")
    return dw if stem else dw.view(Cout, k, k, Cin)


def bn_classes(C):
    """Class (c % 7) of every channel of the "signed" BatchNorm state, see bn_state()."""
    return torch.arange(C) % 7


def dead_channels(C):
    """bool [C]: the channels a "signed" case makes identically zero before BatchNorm (c % 13 == 5): batch variance exactly 0."""
    return torch.arange(C) % 13 == 5


def bn_state(C, generator, kind="positive", beta_std=1.0):
    """(gamma, beta), fp32 on the CPU, drawn from `generator`.
    "positive": gamma = U[0, 1) + 0.5, beta = N(0, 1) * beta_std, the draws the GPU tests made before this helper existed (same
    numbers from the same seeds).
    "signed": the per-channel classes of oracle.resnet50_oracle.signed_bn_affine (control, negative, zero, saturated open, saturated
    closed; beta of the drawn classes is N(0, 0.7^2)); the generator advances exactly as for "positive". Fails when C cannot hold all
    seven classes and one dead channel (dead_channels), so that no case passes vacuously."""
    from oracle import resnet50_oracle as R
    assert kind in ("positive", "signed"), kind
    dev = generator.device            # a test's generator may live on the GPU: drawn there, as that test always did, returned on the CPU
    gamma, noise = (torch.rand(C, generator=generator, device=dev) + 0.5).cpu(), torch.randn(C, generator=generator, device=dev).cpu()
    if kind == "positive":
        return gamma, noise * beta_std
    assert len(set(bn_classes(C).tolist())) == 7 and bool(dead_channels(C).any()), f"C = {C} cannot hold the seven classes + a dead channel"
    return R.signed_bn_affine(gamma, noise * R.SIGNED_BETA_STD)


def saturating(x):
    """Where a test hands gamma / beta of the signed state to a loader as scale / shift: classes 4 and 5 (|scale| 0.05, |shift| 1) hold
    the gate open / closed for EVERY element only while 0.05 |x| < 1. Returns x."""
    assert 0.05 * float(x.abs().max()) < 1.0
    return x


def assert_signed_gates(gate, C, what=""):
    """gate: bool [..., C] (ReLU decisions, mask bits, "maximum > 0" bits) of a signed state WITHOUT a shortcut addend, saturation
    checked by the caller: classes 3 (activation exactly 0) and 5 all off, classes 2 and 4 all on."""
    cls = bn_classes(C)
    g = gate.reshape(-1, C).cpu()
    assert not bool(g[:, (cls == 3) | (cls == 5)].any()), f"{what}: a gate bit is on in a class-3 / class-5 channel"
    assert bool(g[:, (cls == 2) | (cls == 4)].all()), f"{what}: a gate bit is off in a class-2 / class-4 channel"


NET_B, NET_HW, NET_C = 4, 64, 10      # geometry of the whole-network cases on the BatchNorm states below
NET_SEED = {"signed": 41, "zero_init_residual": 43}


def network_case(which):
    """(state_dict, image, labels) of the whole-network BatchNorm-state cases (tests/test_gate_pinned_gpu.py; their CPU anchors in
    tests/test_oracle.py run the same numbers).
    "signed": every BatchNorm layer on the signed state, and the filters o % 13 == 5 of conv1 / conv2 of the first block of each stage
    zeroed (pre-BN channel identically 0, batch variance exactly 0).
    "zero_init_residual": the positive state with every bn3.weight = 0 (torchvision's zero_init_residual=True)."""
    from oracle import resnet50_oracle as R
    gen = torch.Generator().manual_seed(NET_SEED[which])
    sd = R.init_state(NET_C, NET_C, False, generator=gen)
    if which == "signed":
        R.randomize_bn(sd, generator=gen, kind="signed")
        for s in range(1, 5):
            for conv in ("conv1", "conv2"):
                w = sd[f"resnet_base.layer{s}.0.{conv}.weight"]
                w[dead_channels(w.shape[0])] = 0
    else:
        R.randomize_bn(sd, generator=gen)
        for k in sd:
            if k.endswith("bn3.weight"):
                sd[k] = torch.zeros_like(sd[k])
    x = torch.rand(NET_B, 3, NET_HW, NET_HW, generator=gen)
    y = torch.randint(-1, NET_C, (NET_B,), generator=gen)
    return sd, x, y


def hip_gates(model):
    """The ReLU / arg-max decisions of the model's latest forward, in the structure oracle.resnet50_oracle.forward(gates=...)
    takes: {"relu": [49 bool tensors, NCHW], "pool_idx": int64 [B,64,Hp,Wp]} (CPU tensors). Read through the debug entry points of
    the C ABI (include/osi.h, "debug" section), i.e. from the very buffers the backward kernels consume."""
    net, _ = model._last
    lib, dev = N.lib(), model._flat_params.device
    B = next(b for (b, h, w), n in model._nets.items() if n is net)
    relu, pool_idx = [], None
    C, H, W = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for i in range(lib.osi_resnet50_debug_num_gates(net.h)):
        N.check(lib.osi_resnet50_debug_gate_shape(net.h, i, ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)))
        g = torch.empty(B, C.value, H.value, W.value, dtype=torch.uint8, device=dev)
        am = torch.empty(B, C.value, H.value, W.value, dtype=torch.int32, device=dev) if i == 0 else None
        N.check(lib.osi_resnet50_debug_gate(net.h, N.ptr(model._ws), i, N.ptr(g), N.ptr(am), S()), "debug_gate")
        relu.append(g.cpu().bool())
        if am is not None:
            pool_idx = am.cpu().long()
    return {"relu": relu, "pool_idx": pool_idx}


class Fusion(ctypes.Structure):
    """osi_dgrad_fusion of include/osi.h (ABI 4)."""
    _fields_ = [("relu_mask", ctypes.c_void_p), ("y0", ctypes.c_void_p), ("mean0", ctypes.c_void_p), ("invstd0", ctypes.c_void_p),
                ("y1", ctypes.c_void_p), ("mean1", ctypes.c_void_p), ("invstd1", ctypes.c_void_p), ("partials", ctypes.c_void_p),
                ("partials_bytes", ctypes.c_size_t), ("scale0", ctypes.c_void_p), ("shift0", ctypes.c_void_p),
                ("pool_idx", ctypes.c_void_p), ("pool_H", ctypes.c_int), ("pool_W", ctypes.c_int), ("addend_stride", ctypes.c_int)]

"""Dev tool: what the frozen-statistics backward (ABI 12) costs at the benchmark geometry (B = 128, 224 x 224, C = 30, entropic loss),
as interleaved rounds of forward + loss + backward so box drift hits all modes alike:
  train      training mode: batch statistics, full BatchNorm backward (the default step without its optimizer);
  frozen     model.train().freeze_bn(): running statistics, parameter gradients (dy = scale * g in the dgrad epilogues);
  frozen_x   model.eval(), every parameter frozen, x.requires_grad_(): the input-only backward (no reduction, no weight gradient).
  train_x    training mode with x.requires_grad_(): the reference point of frozen_x's stem (dY materialised, osi_stem_dgrad).
Then the frozen in-block input gradient (osi_conv_dgrad_fused_frozen) against the training flavour of the same kernel
(osi_conv_dgrad_fused, gate recomputed, one consumer) per in-block layer shape. Device events around each window.
The table goes to profiles/frozen_backward_b128.txt (or the path given).
usage: python tools/time_frozen_backward.py [rounds] [steps per window] [output path]"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import torch

from openset_imagenet import ResNet50, EntropicOpensetLoss
from openset_imagenet import _native as N

B, H, W, C = 128, 224, 224, 30
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "frozen_backward_b128.txt")

# the in-block input gradients of ResNet-50: (name, spatial size of dx, Cin of dx, Cout, k, stride, launches per step)
LAYERS = [("layer1 conv3", 56, 64, 256, 1, 1, 3), ("layer1 conv2", 56, 64, 64, 3, 1, 3),
          ("layer2.0 conv2", 56, 128, 128, 3, 2, 1), ("layer2 conv3", 28, 128, 512, 1, 1, 4), ("layer2 conv2", 28, 128, 128, 3, 1, 3),
          ("layer3.0 conv2", 28, 256, 256, 3, 2, 1), ("layer3 conv3", 14, 256, 1024, 1, 1, 6), ("layer3 conv2", 14, 256, 256, 3, 1, 5),
          ("layer4.0 conv2", 14, 512, 512, 3, 2, 1), ("layer4 conv3", 7, 512, 2048, 1, 1, 3), ("layer4 conv2", 7, 512, 512, 3, 1, 2)]


class Fusion(ctypes.Structure):
    """osi_dgrad_fusion of include/osi.h"""
    _fields_ = [("relu_mask", ctypes.c_void_p), ("y0", ctypes.c_void_p), ("mean0", ctypes.c_void_p), ("invstd0", ctypes.c_void_p),
                ("y1", ctypes.c_void_p), ("mean1", ctypes.c_void_p), ("invstd1", ctypes.c_void_p), ("partials", ctypes.c_void_p),
                ("partials_bytes", ctypes.c_size_t), ("scale0", ctypes.c_void_p), ("shift0", ctypes.c_void_p),
                ("pool_idx", ctypes.c_void_p), ("pool_H", ctypes.c_int), ("pool_W", ctypes.c_int), ("addend_stride", ctypes.c_int)]


def timed(fn, warm, reps, inner):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / inner)
    return t


def main():
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on an MI355X only")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = ResNet50(C, C, False).to(dev)
    with torch.no_grad():                       # running statistics of a model that has seen data, not the 0 / 1 initialisation
        for name, buf in model.named_buffers():
            if name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
            elif name.endswith("running_mean"):
                buf.normal_(0.0, 0.1)
    loss_fn = EntropicOpensetLoss(C, 1.0)
    x = torch.rand(B, 3, H, W, device=dev)
    y = torch.randint(-1, C, (B,), device=dev)

    def setup(training, frozen, params):
        model.train(training).freeze_bn(frozen)
        for p in model.parameters():
            p.requires_grad_(params)

    def step(want_x):
        xi = x.detach().requires_grad_(want_x)
        loss_fn(model(xi)[0], y).backward()

    modes = {"train": ((True, False, True), False), "frozen": ((True, True, True), False),
             "frozen_x": ((False, False, False), True), "train_x": ((True, False, True), True)}

    def window(mode):
        cfg, want_x = modes[mode]
        setup(*cfg)
        return timed(lambda: step(want_x), 2, 1, STEPS)[0]

    for m in modes:                             # settle the clock
        window(m)
    res = {m: [] for m in modes}
    names = tuple(modes)
    for r in range(ROUNDS):
        for m in (names if r % 2 == 0 else names[::-1]):
            res[m].append(window(m))

    lines = [f"frozen-statistics backward, B = {B}, {H} x {W}, C = {C}, entropic loss; forward + loss + backward, ms per step",
             f"{ROUNDS} interleaved rounds of {STEPS} steps (order reversed every other round), device events", "",
             f"{'mode':<10} {'median':>8} {'min':>8} {'max':>8}   rounds"]
    for m, v in res.items():
        lines.append(f"{m:<10} {statistics.median(v):8.3f} {min(v):8.3f} {max(v):8.3f}   " + " ".join(f"{t:.3f}" for t in v))
    lines += ["", "frozen - train per round: " + " ".join(f"{f - t:+.3f}" for f, t in zip(res["frozen"], res["train"])),
              "frozen_x - train_x per round: " + " ".join(f"{f - t:+.3f}" for f, t in zip(res["frozen_x"], res["train_x"])), ""]

    # the in-block input gradient alone: frozen flavour against the training flavour of the same kernel (random operands)
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
    lines += ["in-block input gradient per layer shape, us per launch (median of 10 windows of 20 launches): training flavour "
              "(osi_conv_dgrad_fused) | frozen (osi_conv_dgrad_fused_frozen) | frozen without sums (input-only)",
              f"{'layer':<16} {'dx':>14} {'k/s':>5} {'n':>2} {'train':>9} {'frozen':>9} {'frozen_x':>9}"]
    tot = [0.0, 0.0, 0.0]
    for name, hw, cin, cout, k, stride, count in LAYERS:
        pad = 1 if k == 3 else 0
        d = N.ConvDesc.make(B, hw, hw, cin, cout, k, stride, pad)
        dy = torch.randn(B, d.Ho, d.Wo, cout, device=dev)
        wk = torch.randn(cout, k, k, cin, device=dev) * 0.05
        y0 = torch.randn(B, hw, hw, cin, device=dev)
        dx = torch.empty_like(y0)
        vec = [torch.rand(cin, device=dev) + 0.5 for _ in range(4)]             # mean, invstd, scale, shift
        pb = lib.osi_conv_dgrad_fused_workspace(ctypes.byref(d))
        parts = torch.empty(pb // 4 + 4, device=dev)
        P = ctypes.c_int()
        f = Fusion(y0=y0.data_ptr(), mean0=vec[0].data_ptr(), invstd0=vec[1].data_ptr(), scale0=vec[2].data_ptr(), shift0=vec[3].data_ptr(),
                   partials=parts.data_ptr(), partials_bytes=pb)
        fx = Fusion(y0=y0.data_ptr(), scale0=vec[2].data_ptr(), shift0=vec[3].data_ptr())
        calls = (lambda: N.check(lib.osi_conv_dgrad_fused(ctypes.byref(d), N.ptr(dy), N.ptr(wk), N.ptr(dx), None, ctypes.byref(f), 0, ctypes.byref(P), st)),
                 lambda: N.check(lib.osi_conv_dgrad_fused_frozen(ctypes.byref(d), N.ptr(dy), N.ptr(wk), N.ptr(dx), ctypes.byref(f), 0, ctypes.byref(P), st)),
                 lambda: N.check(lib.osi_conv_dgrad_fused_frozen(ctypes.byref(d), N.ptr(dy), N.ptr(wk), N.ptr(dx), ctypes.byref(fx), 0, ctypes.byref(P), st)))
        us = [1e3 * statistics.median(timed(fn, 10, 10, 20)) for fn in calls]
        for i in range(3):
            tot[i] += count * us[i]
        lines.append(f"{name:<16} {f'{hw}x{hw}x{cin}':>14} {f'{k}/{stride}':>5} {count:>2} {us[0]:9.1f} {us[1]:9.1f} {us[2]:9.1f}")
    lines.append(f"{'per step (n x)':<16} {'':>14} {'':>5} {'':>2} {tot[0]:9.1f} {tot[1]:9.1f} {tot[2]:9.1f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()

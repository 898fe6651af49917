"""Dev tool: wall-clock of three training steps at the benchmark geometry (B = 128, 224 x 224, C = 30, forward + loss + backward
each) — plain (parameter gradients), with dJ/dimage as well, and input-only (every parameter frozen, x.grad only, the PGD-style
inner step) — measured as interleaved rounds of the three so box drift hits all of them alike; plus osi_stem_dgrad alone.
Device events around each window (ends in a synchronise). usage: python tools/time_input_grad.py [rounds] [steps per window]"""
import json
import os
import statistics
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import torch

from openset_imagenet import ResNet50, EntropicOpensetLoss
from openset_imagenet import _native as N

B, H, W, C = 128, 224, 224, 30
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10


def main():
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on an MI355X only")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = ResNet50(C, C, False).to(dev).train()
    loss_fn = EntropicOpensetLoss(C, 1.0)
    x = torch.rand(B, 3, H, W, device=dev)
    y = torch.randint(-1, C, (B,), device=dev)

    def set_frozen(frozen):
        for p in model.parameters():
            p.requires_grad_(not frozen)

    def step(mode):
        xi = x if mode == "plain" else x.detach().requires_grad_()
        logits, feats = model(xi)
        loss_fn(logits, y).backward()
        return xi

    def window(mode):
        set_frozen(mode == "input_only")
        for _ in range(2):                 # this mode's shapes / plan warm
            step(mode)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            xi = step(mode)
        e1.record()
        torch.cuda.synchronize()
        if mode != "plain" and xi.grad is None:
            raise SystemExit(f"{mode}: the step produced no x.grad")
        return e0.elapsed_time(e1) / STEPS

    modes = ("plain", "with_input_grad", "input_only")
    for m in modes:                         # settle the clock
        window(m)
    res = {m: [] for m in modes}
    for r in range(ROUNDS):
        order = modes if r % 2 == 0 else modes[::-1]
        for m in order:
            res[m].append(window(m))
    set_frozen(False)

    # the kernel alone (same geometry, random dY)
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, Hs, Ws, 64, device=dev)
    wk = torch.randn(64, 7, 7, 3, device=dev) * 0.05
    dx = torch.empty(B, 3, H, W, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    fn = lambda: N.check(N.lib().osi_stem_dgrad(N.ptr(dy), N.ptr(wk), N.ptr(dx), B, H, W, st), "osi_stem_dgrad")
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    kt = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        kt.append(e0.elapsed_time(e1) / 20)
    flop = 2.0 * B * H * W * 3 * 64 * 12.25
    out = {"B": B, "H": H, "W": W, "rounds": ROUNDS, "steps_per_window": STEPS,
           "ms_per_step": {m: {"median": statistics.median(v), "min": min(v), "max": max(v)} for m, v in res.items()},
           "stem_dgrad_ms": {"median": statistics.median(kt), "min": min(kt)},
           "stem_dgrad_gflop": flop / 1e9, "stem_dgrad_tflops_at_median": flop / statistics.median(kt) / 1e9}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

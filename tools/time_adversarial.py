"""Dev tool: wall-clock of the training step with adversarial negatives at the benchmark geometry (B = 128, 224 x 224, C = 30,
entropic loss, Adam), as interleaved rounds of three steps so box drift hits all of them alike:
  plain  forward + loss + backward + Adam step (the default loop's step);
  fused  the FGSM step of train() with cfg.adv.who = fgsm: clean pass whose backward ends in osi_stem_dgrad_fgsm, second forward on
         the model-owned NHWC4 batch, accumulating backward (osi_grad_accumulate), one Adam step;
  hand   the same arithmetic out of the older public pieces: x.requires_grad_(), x.grad, adversary.fgsm_attack (torch ops), second
         forward on the NCHW result, the two arenas summed by torch, mark_gradients_ready(), Adam step.
Plus osi_stem_dgrad_fgsm, osi_stem_dgrad and osi_grad_accumulate alone. Device events around each window (ends in a synchronise).
usage: python tools/time_adversarial.py [rounds] [steps per window]"""
import json
import os
import statistics
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import torch

from openset_imagenet import ResNet50, EntropicOpensetLoss, adversary, optim
from openset_imagenet import _native as N

B, H, W, C = 128, 224, 224, 30
EPS = 8.0 / 255.0
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10


def main():
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on an MI355X only")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = ResNet50(C, C, False).to(dev).train()
    loss_fn = EntropicOpensetLoss(C, 1.0)
    opt = optim.Adam(model, lr=1e-4)
    x = torch.rand(B, 3, H, W, device=dev)
    y = torch.randint(-1, C, (B,), device=dev)
    neg = torch.full_like(y, -1)

    def plain():
        opt.zero_grad()
        loss_fn(model(x)[0], y).backward()
        opt.step()

    def fused():
        opt.zero_grad()
        j = loss_fn(model(x)[0], y)
        model.next_backward(fgsm=EPS)
        j.backward()
        ja = loss_fn(model(model.adversarial_batch())[0], neg)
        model.next_backward(accumulate=True)
        ja.backward()
        opt.step()

    def hand():
        opt.zero_grad()
        xi = x.detach().requires_grad_()
        loss_fn(model(xi)[0], y).backward()
        g1 = model.flat_gradients().clone()
        xn = adversary.fgsm_attack(x, xi.grad, EPS)
        loss_fn(model(xn)[0], neg).backward()
        with torch.no_grad():
            model.flat_gradients().add_(g1)
        model.mark_gradients_ready()
        opt.step()

    steps = {"plain": plain, "fused": fused, "hand": hand}

    def window(mode):
        fn = steps[mode]
        for _ in range(2):                 # this mode's shapes / plan warm
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    modes = tuple(steps)
    for m in modes:                         # settle the clock
        window(m)
    res = {m: [] for m in modes}
    for r in range(ROUNDS):
        order = modes if r % 2 == 0 else modes[::-1]
        for m in order:
            res[m].append(window(m))

    # the kernels alone (same geometry, random operands)
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, Hs, Ws, 64, device=dev)
    wk = torch.randn(64, 7, 7, 3, device=dev) * 0.05
    dx = torch.empty(B, 3, H, W, device=dev)
    x4 = torch.rand(B, H, W, 4, device=dev)
    xa = torch.empty(B, H, W, 4, device=dev)
    ga, gb = torch.zeros_like(model.flat_gradients()), torch.ones_like(model.flat_gradients())
    st = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    kernels = {
        "stem_dgrad_fgsm": lambda: N.check(lib.osi_stem_dgrad_fgsm(N.ptr(dy), N.ptr(wk), N.ptr(x4), N.ptr(xa), EPS, 0.0, 1.0, B, H, W, st)),
        "stem_dgrad": lambda: N.check(lib.osi_stem_dgrad(N.ptr(dy), N.ptr(wk), N.ptr(dx), B, H, W, st)),
        "grad_accumulate": lambda: N.check(lib.osi_grad_accumulate(N.ptr(ga), N.ptr(gb), ga.numel(), st)),
    }
    kt = {}
    for name, fn in kernels.items():
        for _ in range(30):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / 20)
        kt[name] = {"median": statistics.median(t), "min": min(t)}
    out = {"B": B, "H": H, "W": W, "rounds": ROUNDS, "steps_per_window": STEPS,
           "ms_per_step": {m: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for m, v in res.items()},
           "fused_minus_hand_ms_per_round": [f - h for f, h in zip(res["fused"], res["hand"])],
           "kernel_ms": kt, "grad_accumulate_gb": 3 * 4 * ga.numel() / 1e9}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

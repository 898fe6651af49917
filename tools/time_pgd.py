"""Dev tool: the two timings of the projected-attack path at the benchmark geometry (B = 128, 224 x 224, C = 30, entropic loss), HIP
events around windows that end in a synchronise, the two sides of each comparison alternating round by round so box drift hits both:
  kernels  osi_stem_dgrad_pgd against osi_stem_dgrad_fgsm (random operands; the PGD form reads one more NHWC4 batch, the anchor);
  pass     one input-only attack pass — frozen-statistics forward + osi_resnet50_backward_attack(param_grads = 0), what every inner
           PGD step and every attack inside validate() costs — against the same forward + the full osi_resnet50_backward_adv, which
           was the only backward ending in an attack epilogue before.
usage: python tools/time_pgd.py [rounds] [passes per window]"""
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
EPS, ALPHA = 8.0 / 255.0, 2.0 / 255.0
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(sides, n, warm):
    """{name: [ms per call, one per round]}: every round times each side once, the order reversed every other round"""
    names = tuple(sides)
    for name in names:
        for _ in range(warm):
            sides[name]()
    torch.cuda.synchronize()
    res = {name: [] for name in names}
    for r in range(ROUNDS):
        for name in (names if r % 2 == 0 else names[::-1]):
            sides[name]()                      # the side's own operands warm again
            torch.cuda.synchronize()
            res[name].append(timed(sides[name], n))
    return res


def summary(res):
    return {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v} for name, v in res.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on an MI355X only")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    lib = N.lib()
    st = torch.cuda.current_stream().cuda_stream

    # ---- the kernels alone
    Hs, Ws = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, Hs, Ws, 64, device=dev)
    wk = torch.randn(64, 7, 7, 3, device=dev) * 0.05
    x4 = torch.rand(B, H, W, 4, device=dev)
    a4 = torch.rand(B, H, W, 4, device=dev)
    xn = torch.empty(B, H, W, 4, device=dev)
    kernels = {
        "stem_dgrad_fgsm": lambda: N.check(lib.osi_stem_dgrad_fgsm(N.ptr(dy), N.ptr(wk), N.ptr(x4), N.ptr(xn), EPS, 0.0, 1.0, B, H, W, st)),
        "stem_dgrad_pgd": lambda: N.check(lib.osi_stem_dgrad_pgd(N.ptr(dy), N.ptr(wk), N.ptr(x4), N.ptr(a4), N.ptr(xn), ALPHA, EPS, 0.0, 1.0,
                                                                 B, H, W, st)),
        "stem_dgrad_pgd_anchor_is_iterate": lambda: N.check(lib.osi_stem_dgrad_pgd(N.ptr(dy), N.ptr(wk), N.ptr(x4), N.ptr(x4), N.ptr(xn), ALPHA,
                                                                                   EPS, 0.0, 1.0, B, H, W, st)),
    }
    kt = alternate(kernels, 20, 30)
    del dy, wk, a4, xn

    # ---- one attack pass through the model's public route, the iterate an NHWC4 batch bound in place
    model = ResNet50(C, C, False).to(dev).eval()
    loss_fn = EntropicOpensetLoss(C, 1.0)
    y = torch.randint(-1, C, (B,), device=dev)
    anchor = torch.rand(B, H, W, 4, device=dev)

    def input_only():
        model.next_backward(pgd=(ALPHA, EPS, anchor), input_only=True)
        loss_fn(model(x4)[0], y).backward()

    def full_adv():
        model.next_backward(fgsm=EPS)
        loss_fn(model(x4)[0], y).backward()

    pt = alternate({"frozen_forward_plus_attack_input_only": input_only, "frozen_forward_plus_backward_adv": full_adv}, STEPS, 3)
    anchor_bytes = B * H * W * 4 * 4
    out = {"B": B, "H": H, "W": W, "rounds": ROUNDS, "kernel_calls_per_window": 20, "passes_per_window": STEPS,
           "kernel_ms": summary(kt), "pass_ms": summary(pt), "anchor_mb": anchor_bytes / 1e6,
           "pgd_minus_fgsm_ms_per_round": [p - f for p, f in zip(kt["stem_dgrad_pgd"], kt["stem_dgrad_fgsm"])],
           "input_only_over_full_per_round": [a / b for a, b in zip(pt["frozen_forward_plus_attack_input_only"],
                                                                    pt["frozen_forward_plus_backward_adv"])]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

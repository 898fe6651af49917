"""Dev probe: time of one optimizer launch over the full ResNet-50 arena (23.76 M floats), plain against grouped.

Legs, interleaved round by round in one process (HIP events around one launch each; median and spread over the rounds):
  plain            osi_adam_step / osi_sgd_step
  groups 1 seg     osi_*_step_groups, one segment over the whole arena, default options
  groups split     the optim.split_decay table of the model (decay / no-decay, about 110 segments)
  groups amsgrad   (Adam) the split table with amsgrad on: a third state arena, 9 x 4 B per element instead of 7
The yardstick for the grouped legs is the plain leg's own time and its round-to-round spread in the same run.

  python tools/optim_step_probe.py [--rounds 30] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import torch
from openset_imagenet import ResNet50, optim, _native as N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 20
    cuda = torch.device("cuda:0")
    L = N.lib()
    model = ResNet50(116, 116, False)
    n = model.flat_parameters().numel()
    split = optim.AdamW(optim.split_decay(model, 1e-2), lr=1e-3)._plan_for()[1]
    rows = [tuple(split[i:i + 3]) for i in range(0, len(split), 3)]
    seg_split = (N.OptSegment * len(rows))(*[N.OptSegment(*r) for r in rows])
    seg_one = (N.OptSegment * 1)(N.OptSegment(0, n // 4, 0))
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=gen).to(cuda)
    g = (torch.randn(n, generator=gen) * 1e-3).to(cuda)
    m, v, vmax = (torch.zeros(n, device=cuda) for _ in range(3))
    S = torch.cuda.current_stream().cuda_stream
    P = N.ptr

    def adam_groups(seg, nseg, amsgrad):
        gs = (N.AdamGroup * 2)(N.AdamGroup(1e-3, 0.9, 0.999, 1e-8, 1e-2 if amsgrad else 0.0, 5, int(amsgrad), int(amsgrad), 0),
                               N.AdamGroup(1e-3, 0.9, 0.999, 1e-8, 0.0, 5, 0, int(amsgrad), 0))
        return lambda: N.check(L.osi_adam_step_groups(P(p), P(g), P(m), P(v), P(vmax), n, seg, nseg, gs, 2, 1.0, S))

    def sgd_groups(seg, nseg, wd):
        gs = (N.SgdGroup * 2)(N.SgdGroup(1e-3, 0.9, 0.0, wd, 0, 0, 0), N.SgdGroup(1e-3, 0.9, 0.0, 0.0, 0, 0, 0))
        return lambda: N.check(L.osi_sgd_step_groups(P(p), P(g), P(m), n, seg, nseg, gs, 2, 1.0, S))

    legs = [
        ("adam plain", 7, lambda: N.check(L.osi_adam_step(P(p), P(g), P(m), P(v), n, 1e-3, 0.9, 0.999, 1e-8, 5, 1.0, S))),
        ("adam groups 1 seg", 7, adam_groups(seg_one, 1, False)),
        (f"adam groups split ({len(rows)} seg)", 7, adam_groups(seg_split, len(rows), False)),
        (f"adamw groups split + amsgrad ({len(rows)} seg)", 9, adam_groups(seg_split, len(rows), True)),
        ("sgd plain", 5, lambda: N.check(L.osi_sgd_step(P(p), P(g), P(m), n, 1e-3, 0.9, 0, 1.0, S))),
        ("sgd groups 1 seg", 5, sgd_groups(seg_one, 1, 0.0)),
        (f"sgd groups split, wd ({len(rows)} seg)", 5, sgd_groups(seg_split, len(rows), 1e-4)),
    ]
    times = {name: [] for name, _, _ in legs}
    for name, _, fn in legs:          # warm-up: code objects loaded, clocks up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, _, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    lines = [f"arena {n} floats, {args.rounds} interleaved rounds, one launch per leg and round, {torch.cuda.get_device_name(0)}",
             f"{'leg':<48}{'median us':>10}{'min':>9}{'max':>9}{'p10-p90':>10}{'GB/s':>9}"]
    for name, words, _ in legs:
        t = sorted(times[name])
        med = statistics.median(t)
        spread = t[int(0.9 * (len(t) - 1))] - t[int(0.1 * (len(t) - 1))]
        lines.append(f"{name:<48}{med:>10.1f}{t[0]:>9.1f}{t[-1]:>9.1f}{spread:>10.1f}{words * 4 * n / med / 1e3:>9.0f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Dev probe: what gradient-norm clipping costs in front of the fused optimizer step, full ResNet-50 arena (C = 30).

Legs, interleaved round by round in one process (HIP events around one call each; median and spread over the rounds), for Adam and
for SGD, each through the public optimizer objects over random gradients:
  step() A / step() B      the unclipped step, twice: the A/A spread every other difference is read against
  step(clip_norm=inf)      norm + device-scalar step, the clip inactive ("measure only")
  step(clip_norm=active)   the same with the clip active (the same launches: the scalar differs)
  torch clip + step()      torch.nn.utils.clip_grad_norm_ over the arena views, then step(); timed only if it runs on them
  norm only                osi_grad_clip_scale alone over the optimizer's spans (two launches; GB/s of the one arena read)
HIP events around a call that makes several launches include the host's launch gaps: that is the cost a training step sees.

  python tools/clip_step_probe.py [--rounds 30] [--out FILE]
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
    model = ResNet50(30, 30, False).to(cuda)
    n = model.flat_parameters().numel()
    with torch.no_grad():
        model.flat_gradients().copy_((torch.randn(n, generator=torch.Generator().manual_seed(0)) * 1e-3).to(cuda))
    model.mark_gradients_ready()
    model.bind_gradients()
    params = list(model.parameters())
    raw = float(torch.linalg.vector_norm(model.flat_gradients().double()))
    notes, legs = [], []
    for kind, make in (("adam", lambda: optim.Adam(model.parameters(), lr=1e-5)), ("sgd", lambda: optim.SGD(model.parameters(), lr=1e-5, momentum=0.9))):
        opt = make()
        opt.step()                       # state arenas allocated, SGD past its first step
        spans = list(opt._spans)
        ws = torch.empty(int(N.lib().osi_grad_norm_workspace(n)), dtype=torch.uint8, device=cuda)
        out2 = torch.zeros(2, device=cuda)

        def unfused(opt=opt):
            torch.nn.utils.clip_grad_norm_(params, 0.5 * raw)
            opt.step()

        legs += [(f"{kind} step() A", opt.step), (f"{kind} step() B", opt.step),
                 (f"{kind} step(clip_norm=inf)", lambda opt=opt: opt.step(clip_norm=float("inf"))),
                 (f"{kind} step(clip_norm=active)", lambda opt=opt: opt.step(clip_norm=0.5 * raw))]
        try:
            before = model.flat_gradients().clone()
            unfused()
            torch.cuda.synchronize()
            scaled = float(torch.linalg.vector_norm(model.flat_gradients().double())) / raw
            with torch.no_grad():        # clip_grad_norm_ scales the gradients in place: put them back for the other legs
                model.flat_gradients().copy_(before)
            notes.append(f"{kind}: torch.nn.utils.clip_grad_norm_ runs on the arena views (it scaled the arena's norm by {scaled:.4f}; "
                         "the probe puts the gradients back after every call of this leg, outside the timed span)")
            legs.append((f"{kind} torch clip + step()", unfused))
        except Exception as e:           # noqa: BLE001 - whatever torch raises here is the finding
            notes.append(f"{kind}: torch.nn.utils.clip_grad_norm_ does not run on the arena views: {type(e).__name__}: {e}")
        legs.append((f"{kind} norm only ({len(spans) // 2} spans)",
                     lambda spans=spans, ws=ws, out2=out2: N.ops().grad_clip_scale(model.flat_gradients(), spans, N.NORM_L2, 1.0, 1.0, ws, out2)))
    saved = model.flat_gradients().clone()

    def restore(name):
        if "torch clip" in name:
            with torch.no_grad():
                model.flat_gradients().copy_(saved)

    times = {name: [] for name, _ in legs}
    for name, fn in legs:                # warm-up: code objects loaded, clocks up
        for _ in range(3):
            fn()
            restore(name)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
            restore(name)
    lines = [f"arena {n} floats ({4 * n / 1e6:.1f} MB), {args.rounds} interleaved rounds, one call per leg and round, {torch.cuda.get_device_name(0)}",
             f"{'leg':<40}{'median us':>10}{'min':>9}{'max':>9}{'p10-p90':>10}"]
    for name, _ in legs:
        t = sorted(times[name])
        med = statistics.median(t)
        spread = t[int(0.9 * (len(t) - 1))] - t[int(0.1 * (len(t) - 1))]
        extra = f"   {4 * n / med / 1e3:.0f} GB/s" if "norm only" in name else ""
        lines.append(f"{name:<40}{med:>10.1f}{t[0]:>9.1f}{t[-1]:>9.1f}{spread:>10.1f}{extra}")
    text = "\n".join(lines + notes)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

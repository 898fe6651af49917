"""Dev probe: what the weight average (EMA / SWA, openset_imagenet/averaging.py) costs per training step.

bench.py's step loop (its workload table, its synthetic batch, Adam) run twice in interleaved windows in one process:
  plain     forward, loss, backward, optimizer step
  averaged  the same, then AveragedModel.update_parameters(model): one osi_average_update launch
and the launch by itself over the full arenas (HIP events around one launch each), set beside the time its traffic — two reads and one
write of every float — would take at a measured 2R:1W stream rate (--stream-gbs, e.g. the row of profiles/r05_hbm_rates.txt).
Launches per step are counted by a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/time_averaging.py).

  python tools/time_averaging.py [--pairs 6] [--steps 20] [--buffers copy|average] [--stream-gbs 6090] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import torch
import bench
from openset_imagenet import EntropicOpensetLoss, ResNet50, optim, tools
from openset_imagenet.averaging import AveragedModel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6, help="interleaved (plain, averaged) window pairs")
    ap.add_argument("--steps", type=int, default=20, help="steps per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="p2", choices=("p1", "p2"))
    ap.add_argument("--buffers", default="copy", choices=("copy", "average"))
    ap.add_argument("--launches", type=int, default=50, help="timed launches of the kernel by itself")
    ap.add_argument("--stream-gbs", type=float, default=None, help="measured 2R:1W stream rate of the device in GB/s")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = tools.set_device_gpu(0)
    wl = bench.WORKLOADS[args.workload]
    B, C = wl["B"], wl["C"]
    torch.manual_seed(42)
    model = tools.device(ResNet50(C, C, False))
    opt = optim.Adam(model.parameters(), lr=1e-3)
    images, labels = bench.synthetic_batch(B, C, wl["p_neg"], "entropic", dev, 42)
    loss_fn = EntropicOpensetLoss(C, 1.0)
    averaged = AveragedModel(model, kind="ema", decay=0.9998, buffers=args.buffers)

    def step(avg):
        model.train()
        opt.zero_grad()
        logits, _ = model(images)
        loss_fn(logits, labels).backward()
        opt.step()
        if avg:
            averaged.update_parameters(model)

    def window(avg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(avg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for _ in range(args.warmup):
        step(False)
        step(True)
    plain, avgd = [], []
    for _ in range(args.pairs):
        plain.append(window(False))
        avgd.append(window(True))
    # the launch by itself
    us = []
    for _ in range(3 if args.launches else 0):
        averaged.update_parameters(model)
    for _ in range(args.launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); averaged.update_parameters(model); b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    floats = model._flat_params.numel() + (model._flat_buffers.numel() if args.buffers == "average" else 0)
    mb = 12 * floats / 1e6
    med = statistics.median(us) if us else float("nan")
    diffs = [b - a for a, b in zip(plain, avgd)]
    lines = [f"{torch.cuda.get_device_name(0)}, workload {args.workload} (B {B}), buffers: {args.buffers}, {args.pairs} interleaved pairs of {args.steps}-step windows",
             f"step, plain     ms: median {statistics.median(plain):.3f}  windows {' '.join(f'{t:.3f}' for t in plain)}",
             f"step, averaged  ms: median {statistics.median(avgd):.3f}  windows {' '.join(f'{t:.3f}' for t in avgd)}",
             f"averaged - plain per pair, ms: median {statistics.median(diffs):+.3f}  pairs {' '.join(f'{d:+.3f}' for d in diffs)}",
             f"update_parameters calls: {int(averaged.n_averaged)}, optimizer steps: {2 * (args.warmup + args.pairs * args.steps)}"]
    if us:
        lines += [
             f"update_parameters by itself (events, includes the {'buffer copy and the ' if args.buffers == 'copy' else ''}counter copy): "
             f"median {med:.1f} us, min {min(us):.1f}, max {max(us):.1f} over {len(us)} launches; {floats} floats, {mb:.1f} MB moved "
             f"(2 reads + 1 write) = {mb / med * 1e3:.0f} GB/s"]
    if args.stream_gbs and us:
        lines.append(f"at the device's measured 2R:1W stream rate of {args.stream_gbs:.0f} GB/s those {mb:.1f} MB take {mb / args.stream_gbs * 1e3:.1f} us")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Dev tool: PROSER (csrc/proser.hip, openset_imagenet/proser.py) - device time from HIP events (median of 20 after 5 warm calls,
inputs resident on the device) of
  * the mix (osi_mix_rows_pairs) at B = 128 on the layer3 input of a 224 x 224 step ([128, 28 * 28 * 512] fp32; the 64 rows PROSER
    mixes = 32 pairs, the other 64 their own partners), with the bytes it moves (every mixed row read once and written once) as a rate,
    on one buffer again and again (served from the Infinity Cache) and rotating over six buffers (from HBM);
  * the loss (osi_proser_loss_fwd_bwd) at B = 128, C = 116, D = 5, 64 mixed rows;
  * the PROSER training step (draw, mixed forward, dummy classifier, loss, backward through autograd) against the same commit's
    freeze_below("layer3") step without a mix (forward, fused softmax loss, backward), both without the optimizers.
Prints one JSON document. A measurement path that finds no GPU fails.
usage: python tools/time_proser.py [--batch 128]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import PROSER, ResNet50, losses
from openset_imagenet import _native as N


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_proser: no GPU")
    dev = torch.device("cuda:0")
    B, C, D = args.batch, 116, 5
    ops = N.ops()
    gen = np.random.default_rng(0)
    out = {"batch": B}

    # ---- the mix on the layer3 input: the rows PROSER mixes (the first (B // 2) & ~1, a random perfect matching), the rest self-partnered
    L = 28 * 28 * 512
    n_mixed = (B // 2) & ~1
    perm = gen.permutation(n_mixed)
    partner = np.arange(B, dtype=np.int32)
    partner[perm[0::2]], partner[perm[1::2]] = perm[1::2], perm[0::2]
    pt, wt = torch.from_numpy(partner).to(dev), torch.full((B,), 0.4, device=dev)
    moved = 2 * n_mixed * L * 4                          # every mixed row read once and written once
    rate = lambda t: moved / (t["median_ms"] * 1e-3) / 1e12
    x = torch.randn(B, L, device=dev)
    t = timed(lambda: ops.mix_rows_pairs(x, pt, wt))
    out["mix_same_buffer"] = dict(t, rows=B, mixed_rows=n_mixed, floats_per_row=L, bytes_moved=moved, tb_per_s=rate(t),
                                  note="the 103 MB a call touches fit the 256 MiB Infinity Cache: repeated calls are not an HBM rate")
    ring = [x] + [torch.randn(B, L, device=dev) for _ in range(5)]      # 6 x 103 MB touched in turn: every call finds its rows in HBM
    turn = [0]

    def rotating():
        turn[0] = (turn[0] + 1) % len(ring)
        ops.mix_rows_pairs(ring[turn[0]], pt, wt)

    t = timed(rotating, warm=6, reps=24)
    out["mix_rotating_buffers"] = dict(t, buffers=len(ring), bytes_moved=moved, tb_per_s=rate(t))
    del ring

    # ---- the loss
    z, d = torch.randn(B, C, device=dev) * 3, torch.randn(B, D, device=dev) * 3
    y = torch.from_numpy(gen.integers(-1, C, size=B)).to(dev)
    out["loss"] = dict(timed(lambda: ops.proser_loss_fwd_bwd(z, d, y, B // 2, 0.01, 1.0, 1.0, True)), C=C, D=D)
    out["loss_only"] = timed(lambda: ops.proser_loss_fwd_bwd(z, d, y, B // 2, 0.01, 1.0, 1.0, False))

    # ---- the step: PROSER against the plain freeze_below("layer3") step
    model = ResNet50(C, C, False).to(dev).train()
    images = torch.rand(B, 3, 224, 224, device=dev)
    labels = torch.from_numpy(gen.integers(0, C, size=B)).to(dev)
    loss_fn = losses.SoftmaxLoss()
    model.freeze_below("layer3")

    def plain():
        logits, _ = model(images)
        loss_fn(logits, labels).backward()

    out["plain_step_freeze_below_layer3"] = timed(plain)
    proser = PROSER(model, dummy_count=D, mix_at="layer3", generator=gen)

    def step():
        proser.dummy_classifier.zero_grad()
        proser.training_step(images, labels).backward()

    out["proser_step"] = timed(step)
    out["plain_step_again"] = timed(plain)               # alternated: the spread of the comparison
    out["proser_step_minus_plain_ms"] = out["proser_step"]["median_ms"] - 0.5 * (
        out["plain_step_freeze_below_layer3"]["median_ms"] + out["plain_step_again"]["median_ms"])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

"""Timings behind profiles/NOTES_shaping.md, on one MI355X: every entry of the activation-shaping block (include/osi.h, ABI 27) from HIP
events, median of 7 calls after 2 warm ones, beside the same result composed from stock torch device ops in the same process:

    order_stats    two adjacent order statistics of 40 000 x 2048 values          torch: sort of the flattened matrix, two reads
    shape_rows     M = 10 000, F = 2048, keep = 205 (p = 90), all five modes       torch: clamp / topk + scatter + sum + exp
    logit_scores   10 000 x 1000, all three modes                                  torch: logsumexp / max / softmax + max

The torch side runs first, then the kernels, then torch again: the two torch columns bracket the box's drift. Bytes are what the
algorithm must move (computed from the shapes below), as a share of the 6.29 TB/s a float4 copy reaches on this part. Prints one JSON
line at the end.

    python tools/time_shaping.py"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import _native as N  # noqa: E402

HBM_COPY = 6.29e12                            # bytes / s, measured float4 copy
WARM, REPS = 2, 7
dev = torch.device("cuda:0")
torch.manual_seed(0)
ops, lib = N.ops(), N.lib()


def timed(fn):
    """Median, in ms, of REPS event-timed calls after WARM warm ones."""
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


# ---- inputs: ReLU-like rows, as the pooled layer gives them
NROWS, F, M, C, KEEP = 40000, 2048, 10000, 1000, 2048 - int(np.round(2048 * 0.9))
bank = torch.relu(torch.randn(NROWS, F, device=dev)).contiguous()
x = bank[:M].contiguous()
logits = (8 * torch.randn(M, C, device=dev)).contiguous()
n = bank.numel()
h = (n - 1) * 0.9
j = int(h)
clip = 1.0
ws_os = torch.empty(lib.osi_order_stats_workspace(n, 2), dtype=torch.uint8, device=dev)
ws_sh = torch.empty(lib.osi_shape_rows_workspace(M, F), dtype=torch.uint8, device=dev)


def torch_shape(mode):
    if mode == N.SHAPE_REACT:
        return torch.clamp(x, max=clip)
    vals, idx = torch.topk(x, KEEP, dim=1)
    if mode == N.SHAPE_ASH_P:
        return torch.zeros_like(x).scatter_(1, idx, vals)
    s1 = x.sum(dim=1, keepdim=True, dtype=torch.float64)
    if mode == N.SHAPE_ASH_B:
        return torch.zeros_like(x).scatter_(1, idx, (s1 / KEEP).float().expand(-1, KEEP))
    scale = torch.exp(s1 / vals.sum(dim=1, keepdim=True, dtype=torch.float64)).float()
    if mode == N.SHAPE_ASH_S:
        return torch.zeros_like(x).scatter_(1, idx, vals * scale)
    return x * scale


def torch_score(mode):
    if mode == N.SCORE_ENERGY:
        return torch.logsumexp(logits, dim=1)
    if mode == N.SCORE_MAXLOGIT:
        return logits.max(dim=1).values
    return torch.softmax(logits, dim=1).max(dim=1).values


SHAPES = (("react", N.SHAPE_REACT, 0), ("ash_p", N.SHAPE_ASH_P, KEEP), ("ash_b", N.SHAPE_ASH_B, KEEP), ("ash_s", N.SHAPE_ASH_S, KEEP),
          ("scale", N.SHAPE_SCALE, KEEP))
SCORES = (("energy", N.SCORE_ENERGY), ("max_logit", N.SCORE_MAXLOGIT), ("msp", N.SCORE_MSP))
rows = {"order_stats": (lambda: torch.sort(bank.flatten()).values[[j, j + 1]], lambda: ops.order_stats(bank, [j, j + 1], ws_os), 4 * 4 * n)}
for name, mode, keep in SHAPES:
    rows["shape_rows " + name] = (lambda mode=mode: torch_shape(mode), lambda mode=mode, keep=keep: ops.shape_rows(x, mode, keep, clip, ws_sh),
                                  2 * 4 * M * F)
for name, mode in SCORES:
    rows["logit_scores " + name] = (lambda mode=mode: torch_score(mode), lambda mode=mode: ops.logit_scores(logits, mode), 4 * M * C + 4 * M)

# the results are compared before anything is timed (recorded, not asserted: torch.topk breaks a tie at the cut as it likes)
want = torch.sort(bank.flatten()).values[[j, j + 1]]
agree = {"order_stats_equal_sort": bool(torch.equal(ops.order_stats(bank, [j, j + 1], ws_os), want)),
         "react_equal_clamp": bool(torch.equal(ops.shape_rows(x, N.SHAPE_REACT, 0, clip, ws_sh), torch_shape(N.SHAPE_REACT))),
         "ash_p_equal_topk_scatter": bool(torch.equal(ops.shape_rows(x, N.SHAPE_ASH_P, KEEP, clip, ws_sh), torch_shape(N.SHAPE_ASH_P))),
         "scale_max_rel_diff": float(((ops.shape_rows(x, N.SHAPE_SCALE, KEEP, clip, ws_sh) - torch_shape(N.SHAPE_SCALE)).abs().max()
                                      / torch_shape(N.SHAPE_SCALE).abs().max())),
         "energy_max_abs_diff": float((ops.logit_scores(logits, N.SCORE_ENERGY) - torch_score(N.SCORE_ENERGY)).abs().max())}
print(agree, flush=True)

out = {"warm": WARM, "reps": REPS, "order_stats_n": n, "M": M, "F": F, "C": C, "keep": KEEP, "agree": agree, "rows": {}}
first = {k: timed(v[0]) for k, v in rows.items()}
ours = {k: timed(v[1]) for k, v in rows.items()}
second = {k: timed(v[0]) for k, v in rows.items()}
print(f"{'entry':24s} {'torch ms':>10s} {'kernel ms':>10s} {'torch ms':>10s} {'MB moved':>10s} {'of 6.29 TB/s':>13s}")
for k, v in rows.items():
    share = v[2] / (ours[k] * 1e-3) / HBM_COPY
    out["rows"][k] = {"torch_first_ms": first[k], "kernel_ms": ours[k], "torch_second_ms": second[k], "bytes": v[2], "hbm_share": share,
                      "slower_than_both": ours[k] > max(first[k], second[k])}
    print(f"{k:24s} {first[k]:10.4f} {ours[k]:10.4f} {second[k]:10.4f} {v[2] / 1e6:10.1f} {100 * share:12.1f}%")
print(json.dumps(out))

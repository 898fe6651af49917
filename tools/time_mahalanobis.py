"""Dev tool: Mahalanobis scores (csrc/mahalanobis.hip) - device time of the fit's and the scoring's calls from HIP events (median of
7 after 2 warm calls, inputs resident on the device), in one process, clocks untouched:
  means and scatter   N = 100 000 rows, F = 2048, C = 116 (2 N F^2 / 2 fp64 multiply-adds on the lower triangle)
  factor              F = 2048 (Cholesky, inverse, log-determinant; the launch count is printed with it)
  whiten + sqdist     a chunk of M = 4096 rows against C = 116 whitened means
next to the parent commit's osi_evm_distances on a problem with the scatter's full multiply-add count, R = N' = F rows of N columns
(the issue's bar: scatter at most 3 x that call). Prints one JSON document.
usage: python tools/time_mahalanobis.py [N [F [M]]]"""
import json
import os
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import _native as NL

C = 116
dev = torch.device("cuda:0")


def timed(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4))


def run(N, F, M):
    g = torch.Generator(device="cpu").manual_seed(F)
    gt = torch.randint(0, C, (N,), generator=g).to(dev)
    centres = 3 * torch.randn(C, F, generator=g)
    x = torch.relu(torch.randn(N, F, generator=g) + centres[gt.cpu()]).to(dev)        # pooled post-ReLU features are non-negative
    ops, lib = NL.ops(), NL.lib()
    ws = torch.empty(max(lib.osi_maha_workspace(N, C, F), lib.osi_evm_workspace(F, F, N)), dtype=torch.uint8, device=dev)
    out = dict(N=N, F=F, C=C, M=M)
    out["class_means"] = timed(lambda: ops.maha_class_means(x, gt, C, ws))
    means, counts = ops.maha_class_means(x, gt, C, ws)
    S = torch.empty(F, F, dtype=torch.float64, device=dev)
    t = timed(lambda: ops.maha_scatter(x, gt, means, NL.MAHA_WITHIN, False, S, ws))
    t["tflops_lower_triangle"] = round(1.0 * N * F * (F + 64) / t["median_ms"] / 1e9, 2)          # 64-wide tiles on and below the diagonal
    out["scatter"] = t
    # the same multiply-add count in fp32 on the tuned distance kernel: R = N' = F rows, the summed index N long
    a = torch.randn(F, N, generator=g).to(dev)
    d = timed(lambda: ops.evm_distances(a, a, NL.EVM_EUCLIDEAN, ws))
    d["tflops"] = round(2.0 * F * F * N / d["median_ms"] / 1e9, 2)
    out["evm_distances_same_macs"] = d
    out["scatter_over_distances"] = round(t["median_ms"] / d["median_ms"], 3)
    del a
    n = int(counts[C])
    f = timed(lambda: ops.maha_factor(S, 1.0 / n, 0.1, ws))
    panels = (F + 63) // 64
    f["launches"] = 2 + 3 * (panels - 1) + 1 + 2 * panels - 1 + 1
    out["factor"] = f
    L, W, logdet, info = ops.maha_factor(S, 1.0 / n, 0.1, ws)
    out["factor_info"], out["logdet"] = int(info), float(logdet)
    zm = ops.maha_whiten(means[:C].contiguous(), W, ws)
    q = x[:M].contiguous()
    out["whiten_chunk"] = timed(lambda: ops.maha_whiten(q, W, ws))
    out["whiten_chunk"]["tflops_lower_triangle"] = round(1.0 * M * F * (F + 64) / out["whiten_chunk"]["median_ms"] / 1e9, 2)
    z = ops.maha_whiten(q, W, ws)
    out["sqdist_chunk"] = timed(lambda: ops.maha_sqdist(z, zm, None, NL.MAHA_SIM_GAUSS, False, ws))
    out["whiten_plus_sqdist_ms"] = round(out["whiten_chunk"]["median_ms"] + out["sqdist_chunk"]["median_ms"], 4)
    return out


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    N, F, M = (a + [100_000, 2048, 4096][len(a):])[:3]
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), run=run(N, F, M)), indent=1))

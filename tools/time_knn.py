"""Dev tool: deep nearest neighbours (csrc/knn.hip) - device time of osi_knn_topk and osi_knn_class_kth from HIP events (median of 7
after 2 warm calls, the distance matrix resident on the device) next to osi_evm_distances for the same chunk, in one process:
M = 4096 queries against a bank of N = 100 000 rows, F = 2048, C = 116 equal class segments, K = 10 and K = 1000. Reports the two
ratios selection / distances (the issue's bar: at most 0.25 each) and the achieved read bandwidth of the selection kernels over the
M x N x 4 bytes of the matrix. Prints one JSON document.
usage: python tools/time_knn.py [M [N [F]]]"""
import json
import os
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import _native as NL

C, KS = 116, (10, 1000)
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


def run(M, N, F):
    g = torch.Generator(device="cpu").manual_seed(F)
    bank = torch.randn(N, F, generator=g).to(dev)
    queries = torch.randn(M, F, generator=g).to(dev)
    start = torch.tensor([N * c // C for c in range(C + 1)], dtype=torch.int64, device=dev)
    ops, lib = NL.ops(), NL.lib()
    ws = torch.empty(max(lib.osi_evm_workspace(M, N, F), lib.osi_knn_workspace(M, N, max(KS))), dtype=torch.uint8, device=dev)
    out = dict(M=M, N=N, F=F, C=C)
    t = timed(lambda: ops.evm_distances(queries, bank, NL.EVM_COSINE, ws))
    t["tflops"] = round(2.0 * M * N * F / t["median_ms"] / 1e9, 2)
    out["distances"] = t
    dist = ops.evm_distances(queries, bank, NL.EVM_COSINE, ws)
    for k in KS:
        a = timed(lambda: ops.knn_topk(dist, k, None, ws))
        b = timed(lambda: ops.knn_class_kth(dist, start, k, None, NL.KNN_SIM_COSINE, ws))
        for r in (a, b):
            r["read_GBps"] = round(M * N * 4 / r["median_ms"] / 1e6, 1)
            r["ratio_to_distances"] = round(r["median_ms"] / t["median_ms"], 4)
        out[f"topk_k{k}"], out[f"class_kth_k{k}"] = a, b
    return out


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    M, N, F = (a + [4096, 100_000, 2048][len(a):])[:3]
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), run=run(M, N, F)), indent=1))

"""Dev tool: ROC-AUC counting (csrc/auc.hip) — device time of osi_auc_binary_f32 / osi_auc_ovr_f32 on device-resident inputs, from HIP
events around a window of calls after a warm-up, plus the wall time of the public functions (allocation, launch, count copy-back,
host division). The result of every timed shape is checked against an exact count on the host first.
usage: python tools/bench_auc.py [N C]...      (default: 20000 116 and 100000 116)"""
import os, sys, time
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import numpy as np
import torch
from openset_imagenet import _native as NV
from openset_imagenet.metrics import auc_score_binary, auc_score_multiclass

shapes = [(int(a), int(b)) for a, b in zip(sys.argv[1::2], sys.argv[2::2])] or [(20000, 116), (100000, 116)]


def exact(pos, neg):
    srt = np.sort(neg)
    lo, hi = np.searchsorted(srt, pos, side="left"), np.searchsorted(srt, pos, side="right")
    return (2 * int(lo.sum()) + int((hi - lo).sum())) / (2 * len(pos) * len(neg))


def events_ms(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def wall_ms(call, reps):
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()                                    # ends in the copy of the counts to the host: synchronous
    return (time.perf_counter() - t0) / reps * 1e3


lib = NV.lib()
for N, C in shapes:
    rng = np.random.default_rng(N)
    z = rng.normal(size=(N, C)) * 3
    s = np.exp(z - z.max(1, keepdims=True)); s = (s / s.sum(1, keepdims=True)).astype(np.float32)
    gb = rng.integers(0, C, size=N); gb[rng.random(N) < 0.4] = -1
    gm = np.concatenate([np.arange(C), rng.integers(0, C, size=N - C)]); rng.shuffle(gm)
    sd, gbd, gmd = torch.from_numpy(s).cuda(), torch.from_numpy(gb).cuda(), torch.from_numpy(gm).cuda()
    m = s.max(1)
    assert auc_score_binary(gbd, sd) == exact(m[gb >= 0], m[gb < 0])
    assert auc_score_multiclass(gmd, sd) == float(np.mean([exact(s[gm == c, c], s[gm != c, c]) for c in range(C)]))
    nb = lib.osi_auc_workspace(N)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    out = torch.zeros(3 * C + 5, dtype=torch.int64, device="cuda")
    st = NV.stream_of(sd)
    binary = lambda: NV.check(lib.osi_auc_binary_f32(NV.ptr(sd), NV.ptr(gbd), N, C, -1, NV.ptr(ws), nb, NV.ptr(out), st))
    ovr = lambda: NV.check(lib.osi_auc_ovr_f32(NV.ptr(sd), NV.ptr(gmd), N, C, NV.ptr(ws), nb, NV.ptr(out[:C]), NV.ptr(out[C:2 * C]),
                                               NV.ptr(out[2 * C:3 * C]), NV.ptr(out[3 * C:]), st))
    reps = 50 if N <= 20000 else 10
    print(f"AUC N={N} C={C} fp32, identical to the exact host count | device time per call (HIP events, {reps} calls after 3): "
          f"binary {events_ms(binary, reps):.3f} ms, one-vs-rest {events_ms(ovr, reps):.3f} ms | wall time of the public functions on "
          f"device-resident inputs: auc_score_binary {wall_ms(lambda: auc_score_binary(gbd, sd), reps):.3f} ms, "
          f"auc_score_multiclass {wall_ms(lambda: auc_score_multiclass(gmd, sd), reps):.3f} ms", flush=True)

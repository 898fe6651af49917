"""Dev tool: detection metrics (csrc/detection.hip) — device time of osi_det_ranks_f32, osi_det_summary and osi_det_curve_f32 on
device-resident inputs, from HIP events around a window of calls after a warm-up, plus the wall time of the public functions
(allocation, launches, copy-back, host divisions) and, where sklearn is installed, the wall time of the four sklearn calls that give
the same figures on the host (roc_auc_score, average_precision_score twice, roc_curve). The result of every timed size is checked
first: against sklearn within 1e-12 where it is there, else against an exact host count of the AUROC.
usage: python tools/bench_detection.py [N]...      (default: 50000)"""
import os, sys, time
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import numpy as np
import torch
from openset_imagenet import _native as NV
from openset_imagenet.metrics import detection_metrics
from openset_imagenet.util import oscr_by_rejection

try:
    from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve
except ImportError:
    roc_auc_score = None

sizes = [int(a) for a in sys.argv[1:]] or [50000]


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
        call()                                    # ends in a copy to the host: synchronous
    return (time.perf_counter() - t0) / reps * 1e3


def sklearn_figures(y, u):
    fpr, tpr, _ = roc_curve(y, -u, drop_intermediate=False)
    return roc_auc_score(y, -u), average_precision_score(y, -u), average_precision_score(1 - y, u), fpr[np.argmax(tpr >= 0.95)]


lib = NV.lib()
for N in sizes:
    rng = np.random.default_rng(N)
    C = 116
    gt = rng.integers(0, C, size=N); gt[rng.random(N) < 0.4] = -2
    u = (rng.normal(size=N) + (gt < 0)).astype(np.float32)
    z = rng.normal(size=(N, C)).astype(np.float32)
    ud, gd, zd = torch.from_numpy(u).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(z).cuda()
    got = detection_metrics(gd, ud)
    host = ""
    if roc_auc_score is not None:
        y = (gt >= 0).astype(np.int64)
        want = sklearn_figures(y, u.astype(np.float64))
        mine = (got["auroc"], got["aupr_in"], got["aupr_out"], got["fpr_at_tpr"][0])
        assert max(abs(a - b) for a, b in zip(mine, want)) <= 1e-12, (mine, want)
        t0 = time.perf_counter()
        for _ in range(3):
            sklearn_figures(y, u.astype(np.float64))
        host = f" | sklearn on the host (4 calls, same figures within 1e-12): {(time.perf_counter() - t0) / 3 * 1e3:.1f} ms"
    else:
        srt = np.sort(u[gt >= 0])
        lo, hi = np.searchsorted(srt, u[gt < 0], side="left"), np.searchsorted(srt, u[gt < 0], side="right")
        assert got["auroc"] == (2 * int(lo.sum()) + int((hi - lo).sum())) / (2 * int((gt >= 0).sum()) * int((gt < 0).sum()))
    nb = lib.osi_det_workspace(N)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ranks = torch.empty((6, N), dtype=torch.int32, device="cuda")
    ints = torch.empty(4 + 3 + 3 + 2 * N, dtype=torch.int64, device="cuda")
    sums, taus = torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float32, device="cuda")
    q = torch.tensor([0.95], dtype=torch.float64, device="cuda")
    correct = (torch.rand(N, device="cuda") < 0.7).to(torch.uint8)
    st = NV.stream_of(ud)
    p = NV.ptr
    f_ranks = lambda: NV.check(lib.osi_det_ranks_f32(p(ud), p(gd), p(correct), N, -2, p(ws), nb, p(ranks), p(ints), st))
    f_summary = lambda: NV.check(lib.osi_det_summary(p(ranks), p(gd), N, -2, p(q), 1, p(ws), nb, p(ints[4:]), p(sums), st))
    f_curve = lambda: NV.check(lib.osi_det_curve_f32(p(ud), p(gd), p(ranks), N, -2, p(ws), nb, p(taus), p(ints[10:]), p(ints[10 + N:]),
                                                     p(ints[7:]), st))
    reps = 20
    print(f"detection N={N} fp32, 40% unknown | device time per call (HIP events, {reps} calls after 3): osi_det_ranks_f32 "
          f"{events_ms(f_ranks, reps):.3f} ms, osi_det_summary {events_ms(f_summary, reps):.3f} ms, osi_det_curve_f32 "
          f"{events_ms(f_curve, reps):.3f} ms | wall time of the public functions on device-resident inputs: detection_metrics "
          f"{wall_ms(lambda: detection_metrics(gd, ud), reps):.3f} ms, oscr_by_rejection (C={C}) "
          f"{wall_ms(lambda: oscr_by_rejection(gd, zd, ud, unk_label=-2), reps):.3f} ms{host}", flush=True)

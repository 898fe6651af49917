"""Dev tool: evaluation histograms (csrc/hist.hip) — wall time of util.get_histogram on device-resident inputs (row values, one copy
of range and counters to the host, numpy edges, two histogram launches, copy-back) next to the numpy restatement of the reference on
host-resident inputs, and the device time of osi_hist_f32 alone from HIP events. Shapes (20000, 116) and (50000, 1000), 30 and 4096
bins, uniform scores and scores that put every known value into one bin. Every timed case is checked against numpy first.
usage: python tools/bench_hist.py"""
import os, sys, time
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import numpy as np
import torch
from openset_imagenet import _native as NV
from openset_imagenet.util import _eval_values, get_histogram


def numpy_histogram(s, gt, bins):
    kn, unk = gt >= 0, gt == -1
    return np.histogram(s[kn, gt[kn]], bins=bins) + np.histogram(np.amax(s[unk], axis=1), bins=bins)


def wall_ms(call, reps):
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()                                    # ends in a copy to the host (or is host code): synchronous
    return (time.perf_counter() - t0) / reps * 1e3


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


lib = NV.lib()
for N, C in ((20000, 116), (50000, 1000)):
    rng = np.random.default_rng(N)
    gt = rng.integers(0, C, size=N); gt[rng.random(N) < 0.4] = -1
    uniform = rng.random((N, C), dtype=np.float32)
    one_bin = uniform * np.float32(0.5)
    one_bin[np.arange(N), np.where(gt >= 0, gt, 0)] = 1.0        # a trained model: every known target score in the top bin
    k = int(np.flatnonzero(gt >= 0)[0])
    one_bin[k, gt[k]] = 0.0                                       # ... but one, so that the range stays [0, 1]
    for tag, s in (("uniform", uniform), ("one bin", one_bin)):
        sd, gd = torch.from_numpy(s).cuda(), torch.from_numpy(gt).cuda()
        for bins in (30, 4096):
            got = get_histogram(dict(scores=sd, gt=gd), bins=bins)
            assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, numpy_histogram(s, gt, bins)))
            kn_val, _, side, _, _ = _eval_values(sd, None, gd, NV.EVAL_SCORE, -1, 0)
            e = torch.from_numpy(got[1].astype(np.float64)).cuda()
            counts = torch.empty(bins, dtype=torch.int64, device="cuda")
            st = NV.stream_of(sd)
            kernel = lambda: NV.check(lib.osi_hist_f32(NV.ptr(kn_val), NV.ptr(side), 1, N, NV.ptr(e), bins, NV.ptr(counts), st))
            reps = 20 if N <= 20000 else 5
            print(f"histogram N={N} C={C} fp32 {tag}, {bins} bins, identical to numpy | get_histogram on device-resident inputs "
                  f"{wall_ms(lambda: get_histogram(dict(scores=sd, gt=gd), bins=bins), reps):.3f} ms | numpy restatement on the host "
                  f"{wall_ms(lambda: numpy_histogram(s, gt, bins), reps):.3f} ms | osi_hist_f32 of the known side alone "
                  f"(HIP events, {reps * 5} calls after 3) {events_ms(kernel, reps * 5):.4f} ms", flush=True)

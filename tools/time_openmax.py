"""Dev tool: OpenMax (csrc/openmax.hip, openset_imagenet/openmax.py) - device time of OpenMax.fit / predict and of every op behind
them from HIP events (median of 10 after 3 warm calls, inputs resident on the device), next to the same arithmetic written in torch on
the device (fp64 index_add / cdist / topk / a vectorised 60-step Newton / scatter / softmax). N = 150 000 rows, C = F = 116 (the
Protocol-1 training split's order of magnitude), tail 1000, alpha 3. The torch version is checked against the kernels first
(shape_rel_diff_vs_torch, probs_abs_diff_vs_torch). Prints one JSON document.
usage: python tools/time_openmax.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import _native as NL
from openset_imagenet.openmax import OpenMax

N, C, F, T, ALPHA = 150_000, 116, 116, 1000, 3
dev = torch.device("cuda:0")
g = torch.Generator(device="cpu").manual_seed(0)
gt = torch.randint(0, C, (N,), generator=g)
gt[torch.rand(N, generator=g) < 0.1] = -1
centres = 3 * torch.randn(C + 1, F, generator=g)
features = (centres[gt.clamp(min=0)] + torch.randn(N, F, generator=g)).float()
logits = torch.randn(N, C, generator=g)
hit = (gt >= 0) & (torch.rand(N, generator=g) < 0.8)
logits[hit, gt[hit]] += 6
features, logits, gt = features.to(dev), logits.to(dev), gt.to(dev)


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


# ------------------------------------------------------------------------------------------------ the same arithmetic in torch
def torch_fit():
    lg_nan = torch.isnan(logits).any(1)
    correct = (gt >= 0) & (gt < C) & ~lg_nan & (logits.argmax(1) == gt)
    y = gt[correct]
    f64 = features[correct].double()
    sums = torch.zeros(C, F, dtype=torch.float64, device=dev).index_add_(0, y, f64)
    count = torch.zeros(C, dtype=torch.int64, device=dev).index_add_(0, y, torch.ones_like(y))
    mav = (sums / count.clamp(min=1)[:, None]).float()
    d = (f64 - mav[y].double()).pow(2).sum(1).sqrt().float()
    tails = torch.full((C, T), float("nan"), dtype=torch.float64, device=dev)
    for c in range(C):
        dc = d[y == c]
        k = min(T, dc.numel())
        tails[c, :k] = dc.topk(k).values.double()
    live = ~torch.isnan(tails)
    shift = torch.where(live, tails, torch.full_like(tails, float("inf"))).min(1).values
    lnx = torch.where(live, (tails - shift[:, None] + 1).log(), torch.zeros_like(tails))
    n = live.sum(1)
    lmax, lmean = lnx.max(1).values, lnx.sum(1) / n
    k = torch.ones(C, dtype=torch.float64, device=dev)
    lo, hi = torch.full_like(k, 1e-3), torch.full_like(k, 1e6)
    for _ in range(60):
        e = torch.where(live, torch.exp(k[:, None] * (lnx - lmax[:, None])), torch.zeros_like(lnx))
        s0, s1, s2 = e.sum(1), (e * lnx).sum(1), (e * lnx * lnx).sum(1)
        m1 = s1 / s0
        gk = m1 - 1 / k - lmean
        lo, hi = torch.where(gk < 0, k, lo), torch.where(gk < 0, hi, k)
        kn = k - gk / (s2 / s0 - m1 * m1 + 1 / (k * k))
        k = torch.where((kn > lo) & (kn < hi), kn, 0.5 * (lo + hi))
    e = torch.where(live, torch.exp(k[:, None] * (lnx - lmax[:, None])), torch.zeros_like(lnx))
    lam = torch.exp(lmax) * (e.sum(1) / n).pow(1 / k)
    return mav, k, lam, shift


def torch_predict(mav, k, lam, shift):
    d = torch.cdist(features.double(), mav.double()).float().double()
    z = d - shift[None, :] + 1
    w = torch.where(z > 0, 1 - torch.exp(-(z.clamp(min=1e-300) / lam[None, :]).pow(k[None, :])), torch.zeros_like(z)).float().double()
    v = logits.double()
    a = min(ALPHA, C)
    top = v.topk(a, dim=1).indices
    ranks = torch.arange(a, device=dev, dtype=torch.float64)
    om = torch.ones_like(v).scatter_(1, top, 1 - w.gather(1, top) * (a - ranks)[None, :] / a)
    hat = torch.cat([v * om, (v * (1 - om)).sum(1, keepdim=True)], 1)
    return torch.softmax(hat, 1).float()


out = dict(N=N, C=C, F=F, tailsize=T, alpha=ALPHA, device=torch.cuda.get_device_name(0))
om = OpenMax(tailsize=T, distance="euclidean", alpha=ALPHA)
om.fit(features, logits, gt)
p_hip = om.predict(logits, features)
state = torch_fit()
p_torch = torch_predict(*state)
torch.cuda.synchronize()
out["fitted_classes"] = int(om.fitted.sum())
out["correct_rows"] = int(om.count.sum())
out["shape_rel_diff_vs_torch"] = float(((om.shape - state[1]).abs() / state[1]).max())
out["probs_abs_diff_vs_torch"] = float((p_hip - p_torch).abs().max())

ops = NL.ops()
ws = om._ws
mav, count, correct = ops.openmax_class_means(features, logits, gt, ws)
d_own = ops.openmax_distances(features, mav, gt, 0)
d_all = ops.openmax_distances(features, mav, None, 0)
w = ops.openmax_wscores(d_all, om.shape, om.scale, om.shift, om.fitted)
t0 = time.time()
out["hip"] = dict(
    fit=timed(lambda: om.fit(features, logits, gt)),
    predict=timed(lambda: om.predict(logits, features)),
    class_means=timed(lambda: ops.openmax_class_means(features, logits, gt, ws)),
    distances_own=timed(lambda: ops.openmax_distances(features, mav, gt, 0)),
    fit_tails=timed(lambda: ops.openmax_fit_tails(d_own, gt, correct, C, T, ws)),
    distances_all=timed(lambda: ops.openmax_distances(features, mav, None, 0)),
    distances_all_cosine=timed(lambda: ops.openmax_distances(features, mav, None, 1)),
    wscores=timed(lambda: ops.openmax_wscores(d_all, om.shape, om.scale, om.shift, om.fitted)),
    recalibrate=timed(lambda: ops.openmax_recalibrate(logits, w, ALPHA)),
)
out["torch"] = dict(fit=timed(torch_fit, warm=2, reps=5), predict=timed(lambda: torch_predict(*state), warm=2, reps=5))
out["timing_wall_s"] = time.time() - t0
print(json.dumps(out, indent=1))

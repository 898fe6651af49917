"""Dev tool: the Extreme Value Machine (csrc/evm.hip, openset_imagenet/evm.py) - device time of the pairwise distance kernel, the
per-row tail fit, the set cover and EVM.fit / predict from HIP events (median of 5 after 2 warm calls, inputs resident on the device),
next to the same fit / predict written in torch on the device (normalised rows, `a @ b.T`, `topk`, a vectorised 60-step Newton, a
per-class maximum). N = 40 000 rows, C = 30 classes of about 1 300 rows (Protocol 2's order of magnitude), tail 1000, cosine, for
F = 30 (the package's own feature width) and F = 2048. For the pairwise kernel it reports the achieved TFLOP/s against the 157.3
nominal fp32 matrix peak and the achieved store bandwidth of `dist`. Prints one JSON document.
usage: python tools/time_evm.py [F ...]"""
import json
import os
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import _native as NL
from openset_imagenet.evm import EVM

N, C, T, M, MULT, PEAK_TF = 40_000, 30, 1000, 10_000, 0.5, 157.3
dev = torch.device("cuda:0")


def timed(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4))


def weibull_torch(tails):
    """Vectorised fit of x = y - min + 1 over the rows of tails [R, T] (fp64): 60 safeguarded Newton steps."""
    shift = tails.min(1).values
    lnx = (tails - shift[:, None] + 1).log()
    lmax, lmean = lnx.max(1).values, lnx.mean(1)
    k = torch.ones_like(shift)
    lo, hi = torch.full_like(k, 1e-3), torch.full_like(k, 1e6)
    for _ in range(60):
        e = torch.exp(k[:, None] * (lnx - lmax[:, None]))
        s0, s1, s2 = e.sum(1), (e * lnx).sum(1), (e * lnx * lnx).sum(1)
        m1 = s1 / s0
        gk = m1 - 1 / k - lmean
        lo, hi = torch.where(gk < 0, k, lo), torch.where(gk < 0, hi, k)
        kn = k - gk / (s2 / s0 - m1 * m1 + 1 / (k * k))
        k = torch.where((kn > lo) & (kn < hi), kn, 0.5 * (lo + hi))
    e = torch.exp(k[:, None] * (lnx - lmax[:, None]))
    return k, torch.exp(lmax) * e.mean(1).pow(1 / k), shift


def run(F):
    g = torch.Generator(device="cpu").manual_seed(F)
    gt = torch.randint(0, C, (N,), generator=g)
    gt[torch.rand(N, generator=g) < 0.1] = -1
    centres = torch.randn(C + 1, F, generator=g)
    features = (centres[gt.clamp(min=0)] + torch.randn(N, F, generator=g)).float().to(dev)
    queries = (centres[torch.randint(0, C + 1, (M,), generator=g)] + torch.randn(M, F, generator=g)).float().to(dev)
    gt = gt.to(dev)
    ops = NL.ops()
    out = dict(F=F)

    x = features[gt == 0].contiguous()
    R = x.shape[0]
    ws = torch.empty(NL.lib().osi_evm_workspace(R, N, F), dtype=torch.uint8, device=dev)
    t = timed(lambda: ops.evm_distances(x, features, NL.EVM_COSINE, ws))
    t.update(rows=R, tflops=round(2.0 * R * N * F / t["median_ms"] / 1e9, 2), store_GBps=round(R * N * 4 / t["median_ms"] / 1e6, 1))
    t["fraction_of_fp32_matrix_peak"] = round(t["tflops"] / PEAK_TF, 4)
    out["pairwise_one_class"] = t
    out["pairwise_one_class_euclidean"] = timed(lambda: ops.evm_distances(x, features, NL.EVM_EUCLIDEAN, ws))
    out["torch_matmul_one_class"] = timed(lambda: x @ features.T)
    dist = ops.evm_distances(x, features, NL.EVM_COSINE, ws)
    out["fit_rows_one_class"] = timed(lambda: ops.evm_fit_rows(dist, gt, 0, T, MULT, ws))
    shape, scale, shift, fitted = ops.evm_fit_rows(dist, gt, 0, T, MULT, ws)[:4]
    dpp = ops.evm_distances(x, x, NL.EVM_COSINE, ws)
    for thr in (0.5, 1.0):                                  # 1.0: nobody covers anybody, R picks
        c = timed(lambda: ops.evm_set_cover(dpp, shape, scale, shift, fitted, MULT, thr, ws))
        c["picks"] = int(ops.evm_set_cover(dpp, shape, scale, shift, fitted, MULT, thr, ws)[1])
        out[f"set_cover_one_class_threshold_{thr}"] = c
    del dist, dpp

    evm = EVM(tailsize=T, cover_threshold=None, distance_multiplier=MULT, distance="cosine")
    out["fit"] = timed(lambda: evm.fit(features, gt), warm=1, reps=3)
    out["extreme_vectors"] = int(evm.ev_start[-1])
    out["predict_10000"] = timed(lambda: evm.predict(queries), warm=1, reps=3)
    cov = EVM(tailsize=T, cover_threshold=0.5, distance_multiplier=MULT, distance="cosine")
    out["fit_with_cover_0.5"] = timed(lambda: cov.fit(features, gt), warm=1, reps=3)
    out["extreme_vectors_with_cover_0.5"] = int(cov.ev_start[-1])
    out["predict_10000_with_cover_0.5"] = timed(lambda: cov.predict(queries), warm=1, reps=3)

    # ---------------------------------------------------------------------------------------- the same method in torch
    rows = [torch.nonzero(gt == k).flatten() for k in range(C)]

    def torch_fit():
        fn = features / features.norm(dim=1, keepdim=True)
        model = []
        for k in range(C):
            d = 1 - fn[rows[k]] @ fn.T
            y = -(MULT * d)
            y[:, rows[k]] = -float("inf")
            model.append(weibull_torch(y.topk(T, dim=1).values.double()))
        return fn, [torch.cat([m[j] for m in model]) for j in range(3)]

    def torch_predict(fn, params):
        ev = torch.cat([fn[r] for r in rows])
        k, lam, shift = params
        start = [0]
        for r in rows:
            start.append(start[-1] + len(r))
        qn = queries / queries.norm(dim=1, keepdim=True)
        res = torch.empty(M, C, device=dev)
        for r0 in range(0, M, 2500):
            z = (-(MULT * (1 - qn[r0:r0 + 2500] @ ev.T))).double() - shift[None, :] + 1
            p = torch.where(z > 0, 1 - torch.exp(-(z.clamp(min=1e-300) / lam[None, :]).pow(k[None, :])), torch.zeros_like(z)).float()
            for c in range(C):
                res[r0:r0 + 2500, c] = p[:, start[c]:start[c + 1]].max(1).values
        return res

    fn, params = torch_fit()
    p_torch, p_hip = torch_predict(fn, params), evm.predict(queries)
    out["probs_abs_diff_vs_torch"] = float((p_hip - p_torch).abs().max())
    out["torch_fit"] = timed(torch_fit, warm=1, reps=3)
    out["torch_predict_10000"] = timed(lambda: torch_predict(fn, params), warm=1, reps=3)
    return out


if __name__ == "__main__":
    widths = [int(a) for a in sys.argv[1:]] or [30, 2048]
    print(json.dumps(dict(N=N, C=C, tailsize=T, queries=M, device=torch.cuda.get_device_name(0), runs=[run(F) for F in widths]), indent=1))

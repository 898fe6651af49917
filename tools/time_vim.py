"""Timings behind profiles/NOTES_vim.md, on one MI355X: ViM.fit at F = 2048, N = 50 000 and its parts (second moment, eigensolver),
np.linalg.eigh on the same matrix beside it (for information), scoring rows per second, sweep counts at smaller widths. Host clock around
work that ends in a device synchronise; every repeat is printed, the first of a call is its warm-up. Prints one JSON line at the end.

    python tools/time_vim.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import ViM, _native as N  # noqa: E402
from openset_imagenet.vim import eigh  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
F, NROWS, C = 2048, 50000, 116
sigma = torch.logspace(np.log10(3.0), np.log10(0.05), F, device=dev)
q = torch.linalg.qr(torch.randn(F, F, device=dev))[0]
x = ((torch.randn(NROWS, F, device=dev) * sigma) @ q.T + 0.1).contiguous()
logits = (3 * torch.randn(NROWS, C, device=dev)).contiguous()
gt = torch.randint(0, C, (NROWS,), device=dev)
out = {"F": F, "N": NROWS, "C": C, "threads": torch.get_num_threads()}


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return r, ts


vim = ViM()
_, ts = timed(lambda: vim.fit(x, logits, gt), 3)
out["fit_s"] = ts
out["sweeps"] = vim.sweeps
out["dim"] = vim.dim
print("fit", ts, "sweeps", vim.sweeps, flush=True)

# the parts: second moment, eigensolver
ops = N.ops()
ws = vim._ws                                  # the fit above sized it for NROWS rows
y = torch.zeros(NROWS, dtype=torch.int64, device=dev)
mean = torch.zeros(2, F, dtype=torch.float64, device=dev)
s = torch.empty(F, F, dtype=torch.float64, device=dev)
_, ts = timed(lambda: ops.maha_scatter(x, y, mean, N.MAHA_TOTAL, False, s, ws), 3)
out["scatter_s"] = ts
(w, v, sweeps), ts = timed(lambda: eigh(s), 3)
out["eigh_s"] = ts
out["eigh_sweeps"] = sweeps
print("scatter", out["scatter_s"], "eigh", ts, sweeps, flush=True)

s_host = s.cpu().numpy()
t = time.perf_counter()
wn, vn = np.linalg.eigh(s_host)
out["numpy_eigh_s"] = time.perf_counter() - t
t = time.perf_counter()
wn, vn = np.linalg.eigh(s_host)
out["numpy_eigh_s_second"] = time.perf_counter() - t
wd, vd = w.cpu().numpy(), v.cpu().numpy()
scale = np.linalg.norm(s_host)
out["residual_rel"] = float(np.linalg.norm(s_host @ vd.T - vd.T * wd) / scale)
out["orth"] = float(np.linalg.norm(vd @ vd.T - np.eye(F)))
out["values_rel"] = float(np.abs(wd - wn[::-1]).max() / scale)
out["numpy_residual_rel"] = float(np.linalg.norm(s_host @ vn - vn * wn) / scale)
print("numpy eigh", out["numpy_eigh_s"], out["numpy_eigh_s_second"], "residual", out["residual_rel"], out["orth"], out["values_rel"], flush=True)

for what, fn in (("unknown_score", lambda: vim.unknown_score(x, logits)), ("probabilities", lambda: vim.probabilities(x, logits)),
                 ("residual_norm", lambda: vim.residual_norm(x))):
    fn()
    _, ts = timed(fn, 5)
    out[what + "_s"] = ts
    out[what + "_rows_per_s"] = NROWS / min(ts)
    print(what, ts, flush=True)

# sweep counts at smaller widths
counts = {}
for f in (256, 512, 1024):
    g = torch.randn(3 * f, f, device=dev, dtype=torch.float64) * torch.logspace(0.5, -1.3, f, device=dev, dtype=torch.float64)
    (_, _, sw), ts = timed(lambda: eigh(g.T @ g), 2)
    counts[f] = {"sweeps": sw, "s": ts}
out["smaller"] = counts
print(counts, flush=True)
print(json.dumps(out))

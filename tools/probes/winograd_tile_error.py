#!/usr/bin/env python3
"""How much of the per-kernel parity bound does a Winograd tile size use?  CPU only, numpy only.

Simulates the 3x3 / stride 1 / pad 1 convolution of the four ResNet-50 conv2 shapes as Winograd F(m x m, 3 x 3) with EVERY product,
sum and transform step rounded to fp32 (the arithmetic of csrc/conv_wino.hip: fp32 transforms, an fp32 FMA-free multiply-add chain
over the input channels per transform-domain position), against an fp64 direct convolution, and prints the maximum error divided
by the project's bound  (2e-6 + 6e-8 sqrt(K)) max|ref| + 1e-6,  K = 9 Cin  (tests/test_production_shapes_gpu.py).  A ratio above 1
fails the existing tests. `direct` is the plain fp32 sum over the 9 Cin products in tap-major order.

The transform matrices are built from the interpolation points (Cook-Toom with the point at infinity): A^T and G in closed form,
B^T from the identity  sum_j AT[i][j] G[j][k] BT[j][l] = [l == i + k]  solved in fp64 and snapped to small rationals, then verified.

  python tools/probes/winograd_tile_error.py                    # the table of profiles/NOTES_r07.md
  python tools/probes/winograd_tile_error.py --points 0,1,-1,0.5,-2 --m 4
"""
import argparse
from fractions import Fraction

import numpy as np

F32 = np.float32
POINTS = {2: [0, 1, -1], 3: [0, 1, -1, 2], 4: [0, 1, -1, 2, -2]}      # the standard sets (Lavin & Gray); + infinity
ALT4 = [0, 1, -1, 0.5, -2]                                             # best alternative tried for F(4x4)


def matrices(m, pts, r=3):
    n = m + r - 1
    a = np.array(pts, dtype=np.float64)
    assert len(a) == n - 1 and len(set(pts)) == n - 1
    AT = np.zeros((m, n)); G = np.zeros((n, r))
    for j in range(n - 1):
        Nj = np.prod([a[j] - a[l] for l in range(n - 1) if l != j])
        AT[:, j] = a[j] ** np.arange(m)
        G[j, :] = a[j] ** np.arange(r) / Nj
    AT[m - 1, n - 1] = 1.0
    G[n - 1, r - 1] = 1.0
    BT = np.zeros((n, n))
    for l in range(n):
        rows, rhs = [], []
        for i in range(m):
            for k in range(r):
                rows.append(AT[i, :] * G[:, k]); rhs.append(1.0 if l == i + k else 0.0)
        BT[:, l] = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
    snap = np.vectorize(lambda v: float(Fraction(v).limit_denominator(4096)))
    AT, G, BT = snap(AT), snap(G), snap(BT)
    d, g = np.random.default_rng(0).standard_normal(n), np.random.default_rng(1).standard_normal(r)
    want = np.array([sum(d[i + k] * g[k] for k in range(r)) for i in range(m)])
    assert np.abs(AT @ ((G @ g) * (BT @ d)) - want).max() < 1e-9, "transform matrices do not reproduce the correlation"
    return AT, G, BT


def xform32(M, x, axis):
    """sum_j M[i][j] x[j] along `axis`, left to right, every product and sum rounded to fp32; zeros skipped, +-1 not multiplied."""
    x = np.moveaxis(x, axis, 0)
    out = []
    for i in range(M.shape[0]):
        acc = None
        for j in range(M.shape[1]):
            c = M[i, j]
            if c == 0.0:
                continue
            t = x[j] if c == 1.0 else (-x[j] if c == -1.0 else (F32(c) * x[j]).astype(F32))
            acc = t if acc is None else (acc + t).astype(F32)
        out.append(acc if acc is not None else np.zeros_like(x[0]))
    return np.moveaxis(np.stack(out).astype(F32), 0, axis)


def wino32(x, w, m, pts):
    """x [H][W][Cin] fp32 (H, W multiples of m), w [Cout][3][3][Cin] fp32 -> y [H][W][Cout] fp32"""
    AT, G, BT = matrices(m, pts)
    n = m + 2
    H, W, Cin = x.shape
    Cout = w.shape[0]
    xp = np.zeros((H + 2, W + 2, Cin), F32); xp[1:-1, 1:-1] = x
    U = xform32(G, xform32(G, w, 1), 2)                                     # [Cout][n][n][Cin]
    y = np.zeros((H, W, Cout), F32)
    for th in range(H // m):
        for tw in range(W // m):
            d = xp[th * m:th * m + n, tw * m:tw * m + n]                    # [n][n][Cin]
            V = xform32(BT, xform32(BT, d, 0), 1)
            M = np.zeros((Cout, n, n), F32)
            for k in range(Cin):                                            # the fp32 chain over the input channels
                M = (M + (U[..., k] * V[None, :, :, k]).astype(F32)).astype(F32)
            Y = xform32(AT, xform32(AT, M, 1), 2)                           # [Cout][m][m]
            y[th * m:th * m + m, tw * m:tw * m + m] = np.moveaxis(Y, 0, 2)
    return y


def direct(x, w, dtype):
    H, W, Cin = x.shape
    xp = np.zeros((H + 2, W + 2, Cin), dtype); xp[1:-1, 1:-1] = x
    y = np.zeros((H, W, w.shape[0]), dtype)
    for r in range(3):
        for s in range(3):
            for k in range(Cin):
                y = (y + (xp[r:r + H, s:s + W, k, None] * w[None, None, :, r, s, k]).astype(dtype)).astype(dtype)
    return y


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--m", type=int, default=0, help="one tile size (2, 3 or 4) instead of the table")
    ap.add_argument("--points", default="", help="finite interpolation points, comma separated (m + 1 of them)")
    ap.add_argument("--hw", type=int, default=12, help="image size of the simulation (a multiple of 12)")
    ap.add_argument("--cout", type=int, default=8)
    a = ap.parse_args()
    forms = [("F(2x2)", 2, POINTS[2]), ("F(3x3)", 3, POINTS[3]), ("F(4x4) std", 4, POINTS[4]), ("F(4x4) alt", 4, ALT4)]
    if a.m:
        forms = [(f"F({a.m}x{a.m})", a.m, [float(v) for v in a.points.split(",")] if a.points else POINTS[a.m])]
    print(f"{'Cin':>4} {'input':>9} {'direct':>8} " + " ".join(f"{n:>11}" for n, _, _ in forms) + "    (max error / bound)")
    for cin in (64, 128, 256, 512):
        for kind in ("relu", "gauss"):
            rng = np.random.default_rng(cin * 7 + (kind == "relu"))
            x = rng.standard_normal((a.hw, a.hw, cin)) * 1.2 + 0.3
            if kind == "relu":
                x = np.maximum(x, 0.0)
            x = x.astype(F32)
            w = (rng.standard_normal((a.cout, 3, 3, cin)) / np.sqrt(9 * cin)).astype(F32)
            ref = direct(x.astype(np.float64), w.astype(np.float64), np.float64)
            bound = (2e-6 + 6e-8 * np.sqrt(9 * cin)) * np.abs(ref).max() + 1e-6
            cells = [np.abs(direct(x, w, F32) - ref).max() / bound]
            cells += [np.abs(wino32(x, w, m, pts) - ref).max() / bound for _, m, pts in forms]
            print(f"{cin:>4} {kind:>9} {cells[0]:8.3f} " + " ".join(f"{c:11.3f}" for c in cells[1:]), flush=True)


if __name__ == "__main__":
    main()

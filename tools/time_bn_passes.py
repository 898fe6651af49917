"""Dev tool: per-launch time of the element-wise BatchNorm passes at the eleven (C, M) geometries of a training step at batch B, as the
executor calls them: the backward apply behind osi_bn_backward_fused (finalising launch + apply), the forward block-output pass
(osi_bn_apply_relu_mask with a residual) and, where the library has it, the two-consumer backward (osi_bn_backward_fused2) next to the
two single passes it replaces. One library per process (compare builds by running the tool once per build, alternating).
Every launch works on its own buffers out of a ring larger than the Infinity Cache, so the rates are HBM rates.
usage: python tools/time_bn_passes.py [B]"""
import ctypes, os, sys
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd"), os.path.join(ROOT, "tests")]
import torch
from openset_imagenet import _native as N

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
L = N.lib(); dev = torch.device("cuda"); st = torch.cuda.current_stream().cuda_stream
RING_BYTES = 640 << 20
# (C, H): every BatchNorm geometry of ResNet-50 behind a streaming pass; the last column marks the projection blocks' outputs
GEOS = [(64, 56, 0), (256, 56, 1), (128, 56, 0), (128, 28, 0), (512, 28, 1), (256, 28, 0), (256, 14, 0), (1024, 14, 1), (512, 14, 0),
        (512, 7, 0), (2048, 7, 1)]


def bench(fns):
    """median of 5 windows over the ring of closures, us per call"""
    n = len(fns)
    reps = max(1, 24 // n)
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for f in fns:
                f()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / (reps * n) * 1e3)
    return sorted(ts)[2]


has2 = hasattr(L, "osi_bn_backward_fused2")
print(f"B={B} abi={L.osi_abi_version()} lib={N.LIB_PATH}")
print("   C    M      MB/tensor | bwd fused: us  TB/s | fwd block out: us  TB/s | two single bwd: us | one pair bwd: us  TB/s")
for C, H, proj in GEOS:
    M = B * H * H
    nbytes = M * C * 4
    P = 3
    ring = max(2, min(8, -(-RING_BYTES // (3 * nbytes))))
    rnd = lambda *s: torch.randn(*s, device=dev)
    mean, invstd, gamma, scale, shift = rnd(C), torch.rand(C, device=dev) + 0.5, rnd(C), rnd(C), rnd(C)
    psum = rnd(3, P, C)
    wsb = max(L.osi_bn_backward_workspace(M, C), (2 * 32 * C + 2 * C) * 4 * 2)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    dg, db = torch.empty(2, C, device=dev), torch.empty(2, C, device=dev)
    sets = [(rnd(M, C), rnd(M, C), torch.empty(M, C, device=dev)) for _ in range(ring)]
    mask = torch.empty(L.osi_bn_relu_mask_bytes(M, C), dtype=torch.uint8, device=dev)

    def bwd(g, y, dy, col=0):
        return lambda: N.check(L.osi_bn_backward_fused(N.ptr(g), N.ptr(y), N.ptr(mean), N.ptr(invstd), N.ptr(gamma), N.ptr(psum[0]),
                                                       N.ptr(psum[1 + col]), P, N.ptr(dy), N.ptr(dg[col]), N.ptr(db[col]), M, C, N.ptr(ws), wsb, st))

    def fwd(y, r, o):
        return lambda: N.check(L.osi_bn_apply_relu_mask(N.ptr(y), N.ptr(r), N.ptr(scale), N.ptr(shift), N.ptr(o), N.ptr(mask), M, C, st))
    t_b = bench([bwd(*s) for s in sets])
    t_f = bench([fwd(*s) for s in sets])
    line = f"{C:5d} {M:7d} {nbytes / 1e6:8.1f}   | {t_b:8.1f} {3 * nbytes / t_b / 1e6:5.2f} | {t_f:8.1f} {3 * nbytes / t_f / 1e6:5.2f} |"
    if proj:
        # a projection block: g -> dy of bn3 and dy of the shortcut's BatchNorm (g, y3, yd read; two dy written)
        sets5 = [(rnd(M, C), rnd(M, C), rnd(M, C), torch.empty(M, C, device=dev), torch.empty(M, C, device=dev))
                 for _ in range(max(2, min(8, -(-RING_BYTES // (5 * nbytes)))))]

        def two(g, y3, yd, d3, dd):
            a, b = bwd(g, yd, dd, 1), bwd(g, y3, d3, 0)
            return lambda: (a(), b())
        t_2 = bench([two(*s) for s in sets5])
        line += f" {t_2:8.1f} |"
        if has2:
            def pair(g, y3, yd, d3, dd):
                tab = (N.BnFusedConsumer * 2)(N.BnFusedConsumer(N.ptr(y3), N.ptr(mean), N.ptr(invstd), N.ptr(gamma), N.ptr(psum[1]), N.ptr(d3), N.ptr(dg[0]), N.ptr(db[0])),
                                              N.BnFusedConsumer(N.ptr(yd), N.ptr(mean), N.ptr(invstd), N.ptr(gamma), N.ptr(psum[2]), N.ptr(dd), N.ptr(dg[1]), N.ptr(db[1])))
                return lambda: N.check(L.osi_bn_backward_fused2(N.ptr(g), tab, N.ptr(psum[0]), P, M, C, N.ptr(ws), wsb, st))
            t_p = bench([pair(*s) for s in sets5])
            line += f" {t_p:8.1f} {5 * nbytes / t_p / 1e6:5.2f}"
        del sets5
    print(line, flush=True)
    del sets
    torch.cuda.empty_cache()

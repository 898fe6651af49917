"""Generates tests/golden/bn_digests.json: SHA-256 digests of everything the BatchNorm entry points of csrc/bn.hip write (outputs, ReLU
bitmask, workspace), recorded from the library built at the commit BEFORE a change to that file, so that tests/test_bn_digests_gpu.py can
recompute them with the library built after it: a refactor of the launch dispatch, the workspace layout or the partial-sum walkers must
leave every bit, and every offset inside a workspace, where it was.

One case per kernel form (CASES), one to three launches each. Inputs come from seeded CPU generators (by shape, so the forms of a shape
see the same tensors) and are copied to the device; every digested buffer is pre-filled with NaN and digested WHOLE (a region that is
not written, or one written somewhere else, changes the digest); the knobs bn_grid, bn_grid_bwd, bn_single_p and bn_wide_p are pinned per
case (KNOBS: their defaults, unless the case names another value) and restored. Nothing in csrc/bn.hip asks for the CU count, so the
digests depend on the chip only through its arithmetic.

    python tests/golden/make_golden_bn_digests.py --parent <hash of the commit the loaded library was built from>
"""
import argparse
import ctypes
import datetime
import functools
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "openset-imagenet_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from openset_imagenet import _native as N  # noqa: E402

OUT = os.path.join(HERE, "bn_digests.json")
KNOBS = dict(bn_grid=1024, bn_grid_bwd=1024, bn_single_p=128, bn_wide_p=2048)      # the defaults of csrc/osi_common.h
BN_GROUPS = 32          # level-1 groups of the two-level reductions: the finalize scratch and a fused2 slice are sized for it
EPS, MOMENTUM = 1e-5, 0.1

# Streamed tensors [M][C]: 5 x 64 is shorter than one tile of 256 float4; C = 64 keeps its coefficients per lane, 96 (24 channel groups)
# takes them per element and leaves idle row lanes in the statistics kernels, 2048 keeps two sets picked by the tile parity and has two
# column groups; a grid of 7 makes every workgroup of the C = 2048 walk see both parities.
STREAM = {"5x64": (5, 64, None), "37x96": (37, 96, None), "37x2048": (37, 2048, None), "37x2048_grid7": (37, 2048, 7)}
STAT_SHAPES = {"37x64": (37, 64), "1031x96": (1031, 96), "5x2048": (5, 2048)}
# Finalisation of [P][C] partials: form -> (knobs, P values). C = 72 is no multiple of 16 (the clamped channel lanes run), two rows per
# partial and M = 2 P - 1 (ragged last tile). rows: 33 runs the unrolled pair loop and its tail. wide: 3 = pivot lanes repeat the last
# tile, 257 = one four-in-flight round plus tail. two-level: 200 = 4 groups of 50 (the 16-lane four-in-flight loop runs once), 2100 = the
# group count capped at 32.
FINAL_C, FINAL_ROWS = 72, 2
FINAL = {"rows": (dict(bn_single_p=128), (1, 17, 33)), "wide": (dict(bn_single_p=1), (3, 70, 257)),
         "two": (dict(bn_single_p=1, bn_wide_p=0), (200, 2100))}
# Backward reducers on seeded [P][C] partials: P -> knobs (one 1024-thread launch, or group sums + one wave per channel)
REDUCE = {3: {}, 70: {}, 257: {}, 200: dict(bn_wide_p=0), 2100: dict(bn_wide_p=0)}
POOL = (2, 9, 64)       # B, H = W, C of the stem-tail backward


def _case(fn, **kw):
    kw.setdefault("knobs", {})
    return dict(fn=fn, **kw)


def _grid(grid):
    return dict(bn_grid=grid, bn_grid_bwd=grid) if grid else {}


CASES = {}
for _n, _s in STAT_SHAPES.items():
    for _r in (0, 1):
        CASES[f"stats_{_n}_run{_r}"] = _case("stats", shape=_s, running=_r)
for _f, (_k, _ps) in FINAL.items():
    for _p in _ps:
        CASES[f"final_{_f}_P{_p}"] = _case("final", P=_p, knobs=_k)
for _n, (_m, _c, _g) in STREAM.items():
    _kw = dict(shape=(_m, _c), knobs=_grid(_g))
    for _res in (0, 1):
        for _relu in (0, 1):
            CASES[f"apply_{_n}_res{_res}_relu{_relu}"] = _case("apply", res=_res, relu=_relu, **_kw)
        CASES[f"apply_mask_{_n}_res{_res}"] = _case("apply_mask", res=_res, **_kw)
    CASES[f"apply_mask2_{_n}"] = _case("apply_mask2", **_kw)
    for _act in (0, 1):
        for _gm in (0, 1):
            CASES[f"bwd_{_n}_act{_act}_gm{_gm}"] = _case("bwd", act=_act, gm=_gm, alias=0, **_kw)
    CASES[f"bwd_{_n}_act1_inplace"] = _case("bwd", act=1, gm=0, alias=1, **_kw)
    for _gm in (0, 1):
        CASES[f"bwd_mask_{_n}_gm{_gm}"] = _case("bwd_mask", gm=_gm, **_kw)
    CASES[f"fused_{_n}_P3"] = _case("fused", P=3, **_kw)
    for _two in (1, 2):
        for _mask in (0, 1):
            for _gm in (0, 1):
                for _pg in (0, 1):
                    CASES[f"frozen_{_n}_n{_two}_mask{_mask}_gm{_gm}_pgrad{_pg}"] = _case("frozen", n=_two, mask=_mask, gm=_gm, pgrad=_pg, **_kw)
for _p, _k in REDUCE.items():
    CASES[f"reduce_C72_P{_p}"] = _case("reduce", P=_p, C=72, knobs=_k)
    if _p != 3:
        CASES[f"fused_37x96_P{_p}"] = _case("fused", P=_p, shape=(37, 96), knobs=_k)
# two consumers; bn_grid_bwd 1024 = the default (the knob's range starts at 1; no cap at 74 tiles), 7 at C = 2048: an odd grid that loops
# falls back to per-element coefficients, 8: an even one keeps one coefficient set per consumer
for _c in (64, 2048):
    for _g in (1024, 7, 8):
        CASES[f"fused2_37x{_c}_grid{_g}"] = _case("fused2", P=3, shape=(37, _c), knobs=dict(bn_grid_bwd=_g))
CASES["fused2_37x64_P257"] = _case("fused2", P=257, shape=(37, 64))
CASES["fused2_37x64_P200_two"] = _case("fused2", P=200, shape=(37, 64), knobs=dict(bn_wide_p=0))
CASES["pool_bwd"] = _case("pool", frozen=0, dy=1, pgrad=1)
CASES["pool_bwd_sums_only"] = _case("pool", frozen=0, dy=0, pgrad=1)
CASES["pool_bwd_frozen"] = _case("pool", frozen=1, dy=1, pgrad=1)
CASES["pool_bwd_frozen_dy_only"] = _case("pool", frozen=1, dy=1, pgrad=0)


def outputs_of(c):
    """The names of the buffers a case digests."""
    fn = c["fn"]
    if fn in ("stats", "final"):
        out = ["mean", "invstd", "scale", "shift", "ws"]
        return out + ["running_mean", "running_var"] if fn == "final" or c["running"] else out
    if fn == "apply":
        return ["out"]
    if fn in ("apply_mask", "apply_mask2"):
        return ["out", "mask"]
    if fn in ("bwd", "bwd_mask"):
        return ["dy", "dgamma", "dbeta", "ws"] + (["gmasked"] if c["gm"] else [])
    if fn == "fused":
        return ["dy", "dgamma", "dbeta", "ws"]
    if fn == "reduce":
        return ["dgamma", "dbeta", "ws"]
    if fn == "fused2":
        return ["dy0", "dy1", "dgamma0", "dgamma1", "dbeta0", "dbeta1", "ws"]
    if fn == "frozen":
        out = ["dy0"] + (["dy1"] if c["n"] == 2 else []) + (["gmasked"] if c["gm"] else [])
        if c["pgrad"]:
            out += ["ws"] + [f"{k}{i}" for k in ("dgamma", "dbeta") for i in range(c["n"])]
        return out
    assert fn == "pool", fn
    return (["dy"] if c["dy"] else []) + (["dgamma", "dbeta", "ws"] if c["pgrad"] else [])


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _nan_bytes(dev, nbytes):
    assert nbytes % 4 == 0
    return _nan(dev, max(nbytes // 4, 1))


@functools.lru_cache(maxsize=None)
def _stream(M, C):
    """CPU tensors of one streamed shape: drawn once, shared by every case of the shape, never written."""
    g = torch.Generator().manual_seed(1000003 * M + C)
    rn, ru = (lambda *s: torch.randn(*s, generator=g)), (lambda *s: torch.rand(*s, generator=g))
    t = dict(y=rn(M, C) * 2 + rn(1, C) * 3, res=rn(M, C), dout=rn(M, C), act=rn(M, C), y2=rn(M, C) * 1.5 + 0.5)
    for k in ("", "2"):     # scales of either sign, as a trained gamma has
        t.update({"scale" + k: ru(C) - 0.3, "shift" + k: rn(C), "mean" + k: rn(C), "invstd" + k: ru(C) + 0.5, "gamma" + k: ru(C) - 0.3})
    t["beta"] = rn(C)
    t["running_mean"], t["running_var"] = rn(C), ru(C) + 0.5
    t["mask"] = torch.randint(0, 256, (N.lib().osi_bn_relu_mask_bytes(M, C),), generator=g, dtype=torch.uint8)
    return t


@functools.lru_cache(maxsize=None)
def _partials(P, C):
    """Seeded [P][C] partial matrices: statistics (means, M2 >= 0) and backward sums (g, g * xhat of two consumers)."""
    g = torch.Generator().manual_seed(7919 * P + C)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(pmean=rn(P, C) * 0.5 + rn(1, C) * 3, pm2=torch.rand(P, C, generator=g) * 2, psum_g=rn(P, C), psum_gx=rn(P, C), psum_gx2=rn(P, C))


class _Dev:
    """t.<name>: the device copy of a CPU tensor of the case's inputs (made on first use)."""

    def __init__(self, dev, cpu):
        self.dev, self.cpu, self.made = dev, cpu, {}

    def __getattr__(self, k):
        if k not in self.made:
            self.made[k] = self.cpu[k].to(self.dev).contiguous()
        return self.made[k]


def _run_stats(lib, dev, c, S):
    M, C = c["shape"]
    t, P = _Dev(dev, _stream(M, C)), N.ptr
    o = {k: _nan(dev, C) for k in ("mean", "invstd", "scale", "shift")}
    if c["running"]:
        o["running_mean"], o["running_var"] = t.running_mean.clone(), t.running_var.clone()
    nb = lib.osi_bn_workspace(M, C)
    o["ws"] = _nan_bytes(dev, nb)
    N.check(lib.osi_bn_train_stats(P(t.y), M, C, P(t.gamma), P(t.beta), EPS, MOMENTUM, P(o.get("running_mean")), P(o.get("running_var")),
                                   P(o["mean"]), P(o["invstd"]), P(o["scale"]), P(o["shift"]), P(o["ws"]), nb, S), "train_stats")
    return o


def _run_final(lib, dev, c, S):
    Pn, C, rows = c["P"], FINAL_C, FINAL_ROWS
    M = rows * Pn - 1
    t, s, P = _Dev(dev, _partials(Pn, C)), _Dev(dev, _stream(37, 96)), N.ptr       # per-channel vectors: the first 72 channels of a streamed shape
    o = {k: _nan(dev, C) for k in ("mean", "invstd", "scale", "shift")}
    o["running_mean"], o["running_var"] = s.running_mean[:C].clone(), s.running_var[:C].clone()
    ws = _nan(dev, 2 * Pn * C + 2 * BN_GROUPS * C)
    ws[:Pn * C] = t.pmean.reshape(-1)
    ws[Pn * C:2 * Pn * C] = t.pm2.reshape(-1)
    o["ws"] = ws
    N.check(lib.osi_bn_finalize_stats(P(ws), ws.numel() * 4, Pn, rows, M, C, P(s.gamma), P(s.beta), EPS, MOMENTUM,
                                      P(o["running_mean"]), P(o["running_var"]), P(o["mean"]), P(o["invstd"]), P(o["scale"]), P(o["shift"]),
                                      S), "finalize_stats")
    return o


def _run_apply(lib, dev, c, S):
    M, C = c["shape"]
    t, P, fn = _Dev(dev, _stream(M, C)), N.ptr, c["fn"]
    o = {"out": _nan(dev, M, C)}
    if fn == "apply":
        N.check(lib.osi_bn_apply(P(t.y), P(t.res) if c["res"] else None, P(t.scale), P(t.shift), P(o["out"]), M, C, c["relu"], S), fn)
        return o
    o["mask"] = _nan_bytes(dev, lib.osi_bn_relu_mask_bytes(M, C))
    if fn == "apply_mask":
        N.check(lib.osi_bn_apply_relu_mask(P(t.y), P(t.res) if c["res"] else None, P(t.scale), P(t.shift), P(o["out"]), P(o["mask"]), M, C, S), fn)
    else:
        N.check(lib.osi_bn_apply_relu_mask2(P(t.y), P(t.scale), P(t.shift), P(t.y2), P(t.scale2), P(t.shift2), P(o["out"]), P(o["mask"]), M, C,
                                            S), fn)
    return o


def _run_bwd(lib, dev, c, S):
    M, C = c["shape"]
    t, P = _Dev(dev, _stream(M, C)), N.ptr
    nb = lib.osi_bn_backward_workspace(M, C)
    o = {"dgamma": _nan(dev, C), "dbeta": _nan(dev, C), "ws": _nan_bytes(dev, nb)}
    if c["gm"]:
        o["gmasked"] = _nan(dev, M, C)
    if c["fn"] == "bwd_mask":
        o["dy"] = _nan(dev, M, C)
        N.check(lib.osi_bn_backward_relu_mask(P(t.dout), P(t.mask), P(t.y), P(t.mean), P(t.invstd), P(t.gamma), P(o["dy"]), P(o.get("gmasked")),
                                              P(o["dgamma"]), P(o["dbeta"]), M, C, P(o["ws"]), nb, S), "backward_relu_mask")
        return o
    dout = t.dout.clone() if c["alias"] else t.dout
    o["dy"] = dout if c["alias"] else _nan(dev, M, C)
    N.check(lib.osi_bn_backward(P(dout), P(t.act) if c["act"] else None, P(t.y), P(t.mean), P(t.invstd), P(t.gamma), P(o["dy"]),
                                P(o.get("gmasked")), P(o["dgamma"]), P(o["dbeta"]), M, C, P(o["ws"]), nb, S), "backward")
    return o


def _run_reduce(lib, dev, c, S):
    Pn, C = c["P"], c["C"]
    t, P = _Dev(dev, _partials(Pn, C)), N.ptr
    o = {"dgamma": _nan(dev, C), "dbeta": _nan(dev, C), "ws": _nan(dev, 2 * BN_GROUPS * C + 2 * C)}
    N.check(lib.osi_bn_backward_reduce(P(t.psum_g), P(t.psum_gx), Pn, P(o["dgamma"]), P(o["dbeta"]), 2 * Pn - 1, C, P(o["ws"]),
                                       o["ws"].numel() * 4, S), "backward_reduce")
    return o


def _run_fused(lib, dev, c, S):
    (M, C), Pn = c["shape"], c["P"]
    t, q, P = _Dev(dev, _stream(M, C)), _Dev(dev, _partials(Pn, C)), N.ptr
    if c["fn"] == "fused":
        o = {"dy": _nan(dev, M, C), "dgamma": _nan(dev, C), "dbeta": _nan(dev, C), "ws": _nan(dev, 2 * BN_GROUPS * C + 2 * C)}
        N.check(lib.osi_bn_backward_fused(P(t.dout), P(t.y), P(t.mean), P(t.invstd), P(t.gamma), P(q.psum_g), P(q.psum_gx), Pn, P(o["dy"]),
                                          P(o["dgamma"]), P(o["dbeta"]), M, C, P(o["ws"]), o["ws"].numel() * 4, S), "backward_fused")
        return o
    nb = lib.osi_bn_backward_fused2_workspace(C)
    o = {f"{k}{i}": _nan(dev, *s) for i in (0, 1) for k, s in (("dy", (M, C)), ("dgamma", (C,)), ("dbeta", (C,)))}
    o["ws"] = _nan_bytes(dev, nb)
    table = (N.BnFusedConsumer * 2)(
        N.BnFusedConsumer(P(t.y), P(t.mean), P(t.invstd), P(t.gamma), P(q.psum_gx), P(o["dy0"]), P(o["dgamma0"]), P(o["dbeta0"])),
        N.BnFusedConsumer(P(t.y2), P(t.mean2), P(t.invstd2), P(t.gamma2), P(q.psum_gx2), P(o["dy1"]), P(o["dgamma1"]), P(o["dbeta1"])))
    N.check(lib.osi_bn_backward_fused2(P(t.dout), table, P(q.psum_g), Pn, M, C, P(o["ws"]), nb, S), "backward_fused2")
    return o


def _run_frozen(lib, dev, c, S):
    M, C = c["shape"]
    t, P, n = _Dev(dev, _stream(M, C)), N.ptr, c["n"]
    o = {f"dy{i}": _nan(dev, M, C) for i in range(n)}
    if c["gm"]:
        o["gmasked"] = _nan(dev, M, C)
    nb = 0
    if c["pgrad"]:
        nb = lib.osi_bn_backward_workspace(M, C)
        o["ws"] = _nan_bytes(dev, nb)
        o.update({f"{k}{i}": _nan(dev, C) for k in ("dgamma", "dbeta") for i in range(n)})
    cons = [N.BnFrozenConsumer(P(t.y), P(t.mean), P(t.invstd), P(t.scale), P(o["dy0"]), P(o.get("dgamma0")), P(o.get("dbeta0"))),
            N.BnFrozenConsumer(P(t.y2), P(t.mean2), P(t.invstd2), P(t.scale2), P(o.get("dy1")), P(o.get("dgamma1")), P(o.get("dbeta1")))]
    table = (N.BnFrozenConsumer * 2)(*cons)
    N.check(lib.osi_bn_backward_frozen(P(t.dout), P(t.mask) if c["mask"] else None, table, n, P(o.get("gmasked")), M, C, P(o.get("ws")), nb,
                                       S), "backward_frozen")
    return o


def _run_pool(lib, dev, c, S):
    B, H, C = POOL
    Ho, M, P = (H - 1) // 2 + 1, B * H * H, N.ptr
    g = torch.Generator().manual_seed(H * 131 + C)
    gpool = torch.randn(B, Ho, Ho, C, generator=g).to(dev)
    # arg-max bytes: tap r * 3 + s of the window, bit 7 = "the window's maximum was positive"
    idx = (torch.randint(0, 9, (B, Ho, Ho, C), generator=g) | (torch.randint(0, 2, (B, Ho, Ho, C), generator=g) << 7)).to(torch.uint8).to(dev)
    y = (torch.randn(M, C, generator=g) * 2 + 0.5).to(dev)
    mean, invstd = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    gamma = (torch.rand(C, generator=g) - 0.3).to(dev)       # the frozen form takes it as scale = gamma * invstd
    o, nb = {}, 0
    if c["dy"]:
        o["dy"] = _nan(dev, M, C)
    if c["pgrad"]:
        nb = lib.osi_bn_backward_workspace(M, C)
        o.update(dgamma=_nan(dev, C), dbeta=_nan(dev, C), ws=_nan_bytes(dev, nb))
    fn = lib.osi_bn_relu_maxpool_bwd_frozen if c["frozen"] else lib.osi_bn_relu_maxpool_bwd
    N.check(fn(P(gpool), P(idx), P(y), P(mean), P(invstd), P(gamma), P(o.get("dy")), P(o.get("dgamma")), P(o.get("dbeta")), B, H, H, C,
               P(o.get("ws")), nb, S), "relu_maxpool_bwd")
    return o


_RUN = {"stats": _run_stats, "final": _run_final, "apply": _run_apply, "apply_mask": _run_apply, "apply_mask2": _run_apply, "bwd": _run_bwd,
        "bwd_mask": _run_bwd, "reduce": _run_reduce, "fused": _run_fused, "fused2": _run_fused, "frozen": _run_frozen, "pool": _run_pool}


def run_case(lib, name, dev):
    """{buffer name: SHA-256} of one case under its pinned knobs."""
    import osi_testlib as T
    c = CASES[name]
    with T.pinned_knobs(**dict(KNOBS, **c["knobs"])):
        bufs = _RUN[c["fn"]](lib, dev, c, T.S())
        got = {k: _sha(v) for k, v in bufs.items()}
    assert sorted(got) == sorted(outputs_of(c)), name
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="hash of the commit the loaded library was built from")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = N.lib()
    cases = {}
    for name in CASES:
        cases[name] = run_case(lib, name, dev)
        assert run_case(lib, name, dev) == cases[name], f"{name}: two runs, two digests"
        print(f"{name}: {cases[name]}")
    props = torch.cuda.get_device_properties(0)
    doc = {"parent_commit": args.parent, "abi_version_recorded": lib.osi_abi_version(), "date": datetime.date.today().isoformat(),
           "recorded_on": f"{props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs)",
           "encoding": "per case: SHA-256 of the raw bytes of each buffer, NaN-prefilled and digested whole (ws = the workspace)",
           "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(cases)} cases")


if __name__ == "__main__":
    main()

"""Generates tests/golden/conv_exit_digests.json: SHA-256 digests of everything the forward and input-gradient convolutions of
csrc/conv_igemm.hip write (output tensor, the used part of the BatchNorm statistics / partial-sum workspace), recorded from the
library built at the commit BEFORE a change to those kernels, so that tests/test_conv_exit_gpu.py can recompute them with the
library built after it: a refactor of the kernels' exit paths (LDS transpose, K-split slab + fix-up, output epilogue, statistics,
row windows) must leave every bit where it was.

One case per kernel form (CASES): inputs come from a seeded CPU generator and are copied to the device, output buffers are pre-filled
with NaN (a row that is not written changes the digest), every shape has a ragged last row tile (M no multiple of 64), and every
plan-relevant knob is pinned — the K split off unless it is the case's subject, and then balanced for a fixed CU count ("tail_cus")
— so the digests do not depend on the chip beyond its arithmetic. A case whose subject is a knob ("off": the knob's other setting)
is run a second time with the knob off: equal digests would make it a blind case, which is dropped and named on stdout and under
"blind". The row walker is the exception ("twin"): it must equal the tile kernel bit for bit, and that equality is what is checked.

    python tests/golden/make_golden_conv_digests.py --parent <hash of the commit the loaded library was built from>
"""
import argparse
import ctypes
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

OUT = os.path.join(HERE, "conv_exit_digests.json")
T64, T64x128, T128x64 = 5, 6, 8      # OSI_TILE_64x64_S1, OSI_TILE_64x128_S1, OSI_TILE_128x64_S1
BASE = dict(tail_split=0, fwd_w3=0, dgrad_w3=0, fwd_rows=0)      # what every case starts from: one plain single-pass launch
SPLIT = dict(tail_split=1, tail_mint=2, tail_smax=32)           # + "tail_cus": short splits allowed, as tests/test_tail_split_gpu.py

# shapes (Cin, Cout, k, stride, H, B)
F1, F3S2, F3 = (128, 64, 1, 1, 14, 3), (256, 128, 3, 2, 9, 5), (128, 128, 3, 1, 9, 3)
R1, R2 = (64, 256, 1, 1, 14, 3), (128, 128, 1, 1, 14, 3)
D1, D3, D3S2 = (64, 64, 1, 1, 14, 3), (128, 64, 3, 1, 9, 3), (256, 128, 3, 2, 9, 2)
DS3, DS2 = (64, 128, 1, 1, 14, 3), (128, 64, 3, 1, 12, 2)       # DCASES[0] / DCASES[4] of tests/test_tail_split_gpu.py (cus 4 / 9)


def _fwd(shape, form, tile=0, knobs=None, off=None, twin=None, split=False):
    return dict(dir="fwd", shape=shape, form=form, tile=tile, knobs=knobs or {}, off=off, twin=twin, split=split)


def _dgrad(shape, flavour, knobs=None, off=None, split=False):
    return dict(dir="dgrad", shape=shape, flavour=flavour, knobs=knobs or {}, off=off, twin=None, split=split)


EPI = {"epi_res_relu": (True, True), "epi_relu": (False, True), "epi_raw": (False, False)}     # form -> (shortcut, ReLU)
CASES = {}
for _n, _s in (("1x1", F1), ("3x3s2", F3S2)):       # the 64x64 tile: plain, fused input activation, the same with a shortcut (1x1 only)
    CASES[f"fwd64_{_n}_stats"] = _fwd(_s, "stats", T64)
    CASES[f"fwd64_{_n}_act"] = _fwd(_s, "act", T64)
CASES["fwd64_1x1_act2"] = _fwd(F1, "act2", T64)
for _f in ("stats", "act"):                         # row windows
    CASES[f"fwd_w3_{_f}"] = _fwd(F3, _f, knobs=dict(fwd_w3=1), off=dict(fwd_w3=0))
CASES["fwd_tile64x128_stats"] = _fwd(F3S2, "stats", T64x128)     # scalar epilogue, two statistics blocks per wave
CASES["fwd_tile128x64_stats"] = _fwd(F3S2, "stats", T128x64)
for _n, _s in (("64to256", R1), ("128to128", R2)):  # row walker: bit for bit the tile kernel
    for _f in ("stats", "act", "epi_res_relu"):
        CASES[f"fwd_rows_{_n}_{_f}"] = _fwd(_s, _f, knobs=dict(fwd_rows=2), twin=dict(fwd_rows=0))
# K split + fix-up: the first two cases of tests/test_tail_split_gpu.py (the second on row windows, its statistics run with the fused input)
CASES["fwd_split_1x1_stats"] = _fwd(F1, "stats", knobs=dict(SPLIT, tail_cus=4), off=dict(tail_split=0), split=True)
CASES["fwd_split_1x1_epi"] = _fwd(F1, "epi_res_relu", knobs=dict(SPLIT, tail_cus=4), off=dict(tail_split=0), split=True)
CASES["fwd_split_w3_act"] = _fwd(F3, "act", knobs=dict(SPLIT, tail_cus=6, fwd_w3=1), off=dict(tail_split=0), split=True)
CASES["fwd_split_w3_epi"] = _fwd(F3, "epi_relu", knobs=dict(SPLIT, tail_cus=6, fwd_w3=1), off=dict(tail_split=0), split=True)
for _f in EPI:                                      # inference epilogue: 64x64 (Cout = 64) and 64x128 (Cout = 128, few tiles) by the plan's rule
    CASES[f"fwd_{_f}_64x64"] = _fwd(F1, _f)
    CASES[f"fwd_{_f}_64x128"] = _fwd(F3S2, _f)
for _fl in range(5):                                # input gradient: plain and the four fused epilogue flavours
    CASES[f"dgrad_1x1_fl{_fl}"] = _dgrad(D1, _fl)
    CASES[f"dgrad_3x3_fl{_fl}"] = _dgrad(D3, _fl)
for _fl in (2, 4):
    CASES[f"dgrad_3x3_w3_fl{_fl}"] = _dgrad(D3, _fl, knobs=dict(dgrad_w3=1), off=dict(dgrad_w3=0))
CASES["dgrad_3x3s2_fl0"] = _dgrad(D3S2, 0)          # four parity classes, some with empty row tiles
CASES["dgrad_3x3s2_fl2"] = _dgrad(D3S2, 2)
CASES["dgrad_split_fl2"] = _dgrad(DS2, 2, knobs=dict(SPLIT, tail_cus=9, dgrad_w3=1), off=dict(tail_split=0), split=True)
CASES["dgrad_split_fl3"] = _dgrad(DS3, 3, knobs=dict(SPLIT, tail_cus=4), off=dict(tail_split=0), split=True)


class _Knobs:
    """Sets knobs on entry, restores what they were on exit."""

    def __init__(self, lib, settings):
        self.lib, self.settings, self.prev = lib, settings, []

    def __enter__(self):
        for k in self.settings:
            v = ctypes.c_int()
            N.check(self.lib.osi_get_tuning(k.encode(), ctypes.byref(v)), k)
            self.prev.append((k, v.value))
        for k, v in self.settings.items():
            N.check(self.lib.osi_set_tuning(k.encode(), v), f"{k} = {v}")

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            N.check(self.lib.osi_set_tuning(k.encode(), v), k)
        return False


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _seed(shape):
    return sum(v * 31 ** i for i, v in enumerate(shape)) % (2 ** 31)


def _run_fwd(lib, dev, c, knobs):
    import osi_testlib as T
    Cin, Cout, k, stride, H, B = c["shape"]
    pad = 1 if k == 3 else 0
    d = N.ConvDesc.make(B, H, H, Cin, Cout, k, stride, pad)
    M = B * d.Ho * d.Wo
    assert M % 64, "every case has a ragged last row tile"
    g = torch.Generator().manual_seed(_seed(c["shape"]))       # by shape alone: the forms of a shape see the same tensors
    x = (torch.randn(B, H, H, Cin, generator=g) + 0.2).to(dev)
    w = (torch.randn(Cout, k, k, Cin, generator=g) / (Cin * k * k) ** 0.5).to(dev)
    isc, ish = (torch.rand(Cin, generator=g) + 0.5).to(dev), (torch.randn(Cin, generator=g) * 0.5).to(dev)
    ires = torch.randn(B, H, H, Cin, generator=g).to(dev)
    osc, osh = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.5).to(dev)
    ores = torch.randn(B, d.Ho, d.Wo, Cout, generator=g).to(dev)
    y = _nan(dev, B, d.Ho, d.Wo, Cout)
    form, P = c["form"], N.ptr
    with _Knobs(lib, knobs):
        if form in EPI:
            nb = lib.osi_conv_fwd_epilogue_workspace(ctypes.byref(d))
            if c["split"] and knobs.get("tail_split"):
                assert nb > 0, "this case is meant to have a split remainder (a slab in the workspace)"
            ws = _nan(dev, max(nb // 4, 4))
            shortcut, relu = EPI[form]
            e = N.ConvEpilogue(osc.data_ptr(), osh.data_ptr(), ores.data_ptr() if shortcut else None, int(relu))
            N.check(lib.osi_conv_fwd_epilogue(ctypes.byref(d), P(x), P(w), P(y), ctypes.byref(e), P(ws) if nb else None, nb, T.S()), form)
            return {"y": _sha(y)}
        nb = lib.osi_conv_fwd_bnstats_workspace(ctypes.byref(d))
        if c["split"] and knobs.get("tail_split"):
            with _Knobs(lib, dict(tail_split=0)):
                assert nb > lib.osi_conv_fwd_bnstats_workspace(ctypes.byref(d)), "this case is meant to have a split remainder"
        ps = _nan(dev, nb // 4)
        np_, rows = ctypes.c_int(), ctypes.c_int()
        tail = (c["tile"], P(ps), nb, ctypes.byref(np_), ctypes.byref(rows), T.S())
        if form == "stats":
            N.check(lib.osi_conv_fwd_bnstats(ctypes.byref(d), P(x), P(w), P(y), *tail), form)
        elif form == "act":
            N.check(lib.osi_conv_fwd_act(ctypes.byref(d), P(x), P(isc), P(ish), P(w), P(y), *tail), form)
        else:
            N.check(lib.osi_conv_fwd_act2(ctypes.byref(d), P(x), P(isc), P(ish), P(ires), P(w), P(y), *tail), form)
        return {"y": _sha(y), "stats": _sha(ps[:2 * np_.value * Cout]), "partials": f"{np_.value} x {rows.value} rows"}


def _run_dgrad(lib, dev, c, knobs):
    import osi_testlib as T
    Cin, Cout, k, stride, H, B = c["shape"]
    pad = 1 if k == 3 else 0
    d = N.ConvDesc.make(B, H, H, Cin, Cout, k, stride, pad)
    M = B * H * H
    assert M % 64, "every case has a ragged last row tile"
    g = torch.Generator().manual_seed(_seed(c["shape"]) + 1)
    dy = torch.randn(B, d.Ho, d.Wo, Cout, generator=g).to(dev)
    w = (torch.randn(Cout, k, k, Cin, generator=g) / (Cout * k * k) ** 0.5).to(dev)
    addend = torch.randn(B, H, H, Cin, generator=g).to(dev)
    y0, y1 = ((torch.randn(M, Cin, generator=g) * 2 + 0.5).to(dev) for _ in range(2))
    mean0, mean1 = ((torch.randn(Cin, generator=g) + 0.5).to(dev) for _ in range(2))
    inv0, inv1 = ((torch.rand(Cin, generator=g) + 0.5).to(dev) for _ in range(2))
    sc, sh = (torch.rand(Cin, generator=g) + 0.5).to(dev), (torch.randn(Cin, generator=g) * 0.5).to(dev)
    mask = torch.randint(0, 256, (lib.osi_bn_relu_mask_bytes(M, Cin),), generator=g, dtype=torch.uint8).to(dev)
    dx = _nan(dev, B, H, H, Cin)
    fl, P = c["flavour"], N.ptr
    with _Knobs(lib, knobs):
        if fl == 0:
            N.check(lib.osi_conv_dgrad(ctypes.byref(d), P(dy), P(w), P(dx), 0, 0, T.S()), "dgrad")
            return {"dx": _sha(dx)}
        pb = lib.osi_conv_dgrad_fused_workspace(ctypes.byref(d))
        if c["split"] and knobs.get("tail_split"):
            with _Knobs(lib, dict(tail_split=0)):
                assert pb > lib.osi_conv_dgrad_fused_workspace(ctypes.byref(d)), "this case is meant to have a split remainder"
        parts = _nan(dev, pb // 4)
        two, gate, bits, add = fl in (1, 3), fl in (1, 2, 4), fl == 3, fl in (1, 3)
        # 1 general (recomputed gate + addend + two consumers), 2 in-block (recomputed gate, one consumer), 3 block input (bitmask, addend,
        # two consumers), 4 = 2 under frozen statistics (plan_dgrad in csrc/conv_igemm.hip)
        f = T.Fusion(P(mask) if bits else None, P(y0), P(mean0), P(inv0), P(y1) if two else None, P(mean1) if two else None,
                     P(inv1) if two else None, P(parts), pb, P(sc) if gate else None, P(sh) if gate else None, None, 0, 0, 0)
        np_ = ctypes.c_int()
        if fl == 4:
            N.check(lib.osi_conv_dgrad_fused_frozen(ctypes.byref(d), P(dy), P(w), P(dx), ctypes.byref(f), 0, ctypes.byref(np_), T.S()), "frozen")
        else:
            N.check(lib.osi_conv_dgrad_fused(ctypes.byref(d), P(dy), P(w), P(dx), P(addend) if add else None, ctypes.byref(f), 0,
                                             ctypes.byref(np_), T.S()), "fused")
        return {"dx": _sha(dx), "sums": _sha(parts[:(3 if two else 2) * np_.value * Cin]), "partials": f"{np_.value} row tiles"}


def run_case(lib, name, dev, override=None):
    """The digests of one case under its own knobs, or with `override` (its "off" / "twin" settings) on top of them."""
    c = CASES[name]
    knobs = dict(BASE, **c["knobs"])
    if override:
        knobs.update(override)
    return (_run_fwd if c["dir"] == "fwd" else _run_dgrad)(lib, dev, c, knobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="hash of the commit the loaded library was built from")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = N.lib()
    cases, blind = {}, []
    for name, c in CASES.items():
        got = run_case(lib, name, dev)
        if c["off"] is not None and run_case(lib, name, dev, c["off"]) == got:
            blind.append(name)
            print(f"{name}: BLIND (equal to the run with {c['off']})")
            continue
        if c["twin"] is not None:
            assert run_case(lib, name, dev, c["twin"]) == got, f"{name}: differs from the run with {c['twin']}"
        cases[name] = got
        print(f"{name}: {got}")
    props = torch.cuda.get_device_properties(0)
    doc = {"parent_commit": args.parent, "abi_version_recorded": lib.osi_abi_version(),
           "recorded_on": f"{props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs)",
           "encoding": "per case: SHA-256 of the raw bytes of each output (y / dx; stats / sums = the used part of the workspace)",
           "cases": cases, "blind": blind}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(cases)} cases kept, dropped as blind: {blind or 'none'}")


if __name__ == "__main__":
    main()

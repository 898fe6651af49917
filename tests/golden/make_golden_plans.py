"""Generates tests/golden/plan_queries.json: what the host-side launch planners of libosi_hip.so answer, recorded from the library
built at the commit BEFORE a change to the planning code, so that tests/test_plan_queries_cpu.py can replay it against the library
built after the change. The workspace queries are pure host arithmetic: no GPU is needed (the library then assumes 256 CUs), and
this recorder refuses to run where a device with another CU count would answer instead.

Recorded per ResNet-50 convolution shape (built the way osi_resnet50_create builds them; B = 128, 64, 8 at 224x224, B = 2 at 64x64):
osi_conv_fwd_bnstats_workspace, osi_conv_fwd_epilogue_workspace, osi_conv_dgrad_fused_workspace (null for the stem) and
osi_conv_wgrad_workspace; and osi_resnet50_workspace_bytes of two executors. All of it under the defaults with tail_cus pinned to 256
and under one changed knob at a time (SETTINGS). dp_reserved_cus only acts through the CU count the plans ask the device for, which
the pin hides: its row is recorded with tail_cus left at 0 and is one of the rows that follow the hardware CU count ("pinned": false).
A setting that changes none of the recorded numbers would be a blind row: it is dropped and named on stdout
(at this recording: tail_gain 0, no ResNet-50 launch of at most tail_qmax rounds models under 8 %; and wgrad_tile 64, whose split
count scales with the tile so that the slab size stays).

    python tests/golden/make_golden_plans.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import _native as N  # noqa: E402

OUT = os.path.join(HERE, "plan_queries.json")
PIN = ("tail_cus", 256)
CONFIGS = ((128, 224, 224), (64, 224, 224), (8, 224, 224), (2, 64, 64))
EXECUTORS = ((128, 224, 224, 116, 116), (2, 64, 64, 5, 5))
SETTINGS = (("tail_split", 0), ("tail_cus", 64), ("tail_smax", 4), ("tail_mint", 8), ("tail_gain", 0), ("tail_qmax", 2),
            ("dp_reserved_cus", 8), ("wgrad_tile", 64), ("wgrad_blocks", 4096), ("wgrad3", 0), ("wgrad3", 1), ("wgrad3_blocks", 256),
            ("wgrad_group", 0), ("stem_direct", 0))
UNPINNED = ("dp_reserved_cus",)      # recorded without the pin: they act on the device's CU count
QUERIES = ("osi_conv_fwd_bnstats_workspace", "osi_conv_fwd_epilogue_workspace", "osi_conv_dgrad_fused_workspace", "osi_conv_wgrad_workspace")


def resnet50_shapes(B, H, W):
    """(B, H, W, Cin, Cout, k, stride, pad) of every convolution, in the executor's order, duplicates dropped."""
    out = [(B, H, W, 4, 64, 7, 2, 3)]
    hs, ws = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    h, w, inpl = (hs + 2 - 3) // 2 + 1, (ws + 2 - 3) // 2 + 1, 64
    for planes, nblk, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for b in range(nblk):
            st = stride if b == 0 else 1
            ho, wo = (h + 2 - 3) // st + 1, (w + 2 - 3) // st + 1
            out += [(B, h, w, inpl, planes, 1, 1, 0), (B, h, w, planes, planes, 3, st, 1), (B, ho, wo, planes, planes * 4, 1, 1, 0)]
            if b == 0:
                out.append((B, h, w, inpl, planes * 4, 1, st, 0))
            inpl, h, w = planes * 4, ho, wo
    return list(dict.fromkeys(out))


def answers(lib, shapes):
    """The numbers under the knobs in force: one row of the four queries per shape, then the executors' workspace sizes."""
    conv = []
    for s in shapes:
        d = N.ConvDesc.make(*s)
        stem = s[3] == 4
        conv.append([None if (stem and q == "osi_conv_dgrad_fused_workspace") else getattr(lib, q)(ctypes.byref(d)) for q in QUERIES])
    execs = []
    for e in EXECUTORS:
        h = ctypes.c_void_p()
        N.check(lib.osi_resnet50_create(ctypes.byref(h), *e, 0), "osi_resnet50_create")
        try:
            execs.append(lib.osi_resnet50_workspace_bytes(h))
        finally:
            lib.osi_resnet50_destroy(h)
    return {"conv": conv, "executors": execs}


def get(lib, name):
    v = ctypes.c_int()
    N.check(lib.osi_get_tuning(name.encode(), ctypes.byref(v)), name)
    return v.value


def under(lib, knobs, shapes):
    """answers() under `knobs` ((name, value) pairs, applied in order); every knob touched is restored."""
    prev = [(k, get(lib, k)) for k, _ in knobs]
    try:
        for k, v in knobs:
            N.check(lib.osi_set_tuning(k.encode(), v), f"{k} = {v}")
        return answers(lib, shapes)
    finally:
        for k, v in reversed(prev):
            N.check(lib.osi_set_tuning(k.encode(), v), k)


def knobs_of(setting):
    """The pin, then the one changed knob (which replaces the pin when it is the pinned knob itself)."""
    if setting is None:
        return [PIN]
    return [tuple(setting)] if setting[0] == PIN[0] or setting[0] in UNPINNED else [PIN, tuple(setting)]


def main():
    import torch
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        sys.exit("a device with other than 256 CUs would answer the CU-following queries: record without one")
    lib = N.lib()
    shapes = [s for c in CONFIGS for s in resnet50_shapes(*c)]
    base = under(lib, knobs_of(None), shapes)
    rows, blind = [], []
    for s in SETTINGS:
        a = under(lib, knobs_of(s), shapes)
        changed = sum(x != y for ra, rb in zip(a["conv"], base["conv"]) for x, y in zip(ra, rb)) + \
            sum(x != y for x, y in zip(a["executors"], base["executors"]))
        print(f"{s[0]} = {s[1]}: {changed} of {4 * len(shapes) + len(EXECUTORS)} numbers differ from the defaults")
        if changed:
            rows.append({"knob": s[0], "value": s[1], "pinned": s[0] not in UNPINNED, **a})
        else:
            blind.append(s)
    doc = {"abi_version_recorded": lib.osi_abi_version(), "pin": list(PIN), "queries": list(QUERIES), "shapes": [list(s) for s in shapes],
           "executor_args": [list(e) for e in EXECUTORS], "defaults": base, "settings": rows}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(shapes)} shapes, {len(rows)} settings kept, dropped as blind: {blind or 'none'}")


if __name__ == "__main__":
    main()

"""Generates tests/golden/exec_schedule.json: the whole-network executor's schedule (which op, in which order, on which stream),
recorded from the library built at the commit BEFORE a change to csrc/resnet50_exec.hip, so that tests/test_exec_schedule_gpu.py can
replay it against the library built after the change. Needs the GPU: the schedule is read back through the executor's timeline
instrumentation (osi_resnet50_profile(net, 2) keeps the side-stream overlap; osi_resnet50_timeline_read returns one (class, on_side)
pair per op — only the times vary from run to run, the pairs do not).

One string per executor call, one character per op: the digit of the op's OSI_PROF class on the caller's stream, the letter
('a' + class) on the side stream. Every executor call opens with the class-0 mark, and the log is read after every call, so call
boundaries are part of the record. The fixture pins op order and stream; it does not see event waits or scratch-buffer identities.

Rows (ROWS): B = 2 at 64 x 64, 10 features / 10 classes on the "signed" state of osi_testlib.network_case; the last row at 72 x 72
(stem output 36 x 36: the fused stem tail is not taken and the materialised route runs). A row whose calls equal those of row "a"
would be a blind row: it is dropped and named on stdout and under "blind" in the file.

    python tests/golden/make_golden_schedule.py --parent <hash of the commit the library was built from>
"""
import argparse
import ctypes
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

OUT = os.path.join(HERE, "exec_schedule.json")
B, HW, C = 2, 64, 10
ALL_UNITS, HEAD = 0x3FFFF, 17
WINO_OFF = (("fwd_wino", 0), ("dgrad_wino", 0), ("wgrad_wino", 0))


def _suffix(unit):
    return (ALL_UNITS >> unit) << unit


def _finetune(tag, frozen):
    fwd = "frozen" if frozen else "train"
    return [(tag[0], dict(fwd=fwd, trainable=(_suffix(14), 0))), (tag[1], dict(fwd=fwd, trainable=(_suffix(14), 14))),
            (tag[2], dict(fwd=fwd, trainable=(1 << HEAD, 0))), (tag[3], dict(fwd=fwd, trainable=(1 << HEAD, HEAD))),
            (tag[4], dict(fwd=fwd, trainable=(ALL_UNITS & ~(1 << 15), 0)))]


# name -> what the row changes from row "a" (training forward + backward in one call, defaults)
ROWS = dict([
    ("a", dict()),
    ("b", dict(options=(("overlap", 0),))),
    ("c", dict(options=(("fwd_fork", 0),))),
    ("d", dict(knobs=WINO_OFF)),
    ("e", dict(options=(("stage_join", 0),), staged=True)),
    ("f", dict(fwd="frozen")),
    ("g", dict(fwd="eval", options=(("eval_fused", 1),), bwd=None)),
    ("h", dict(fwd="eval", options=(("eval_fused", 0),), bwd=None)),
    ("i", dict(bwd="dimage", param_grads=1)),
    ("j", dict(bwd="dimage", param_grads=0)),
    ("k", dict(fwd="frozen", bwd="dimage", param_grads=1)),
    ("l", dict(fwd="frozen", bwd="dimage", param_grads=0)),
    ("m", dict(bwd="adv")),
] + _finetune("nopqr", False) + _finetune("stuvw", True) + [
    ("x", dict(hw=72)),
])


class Case:
    """The arenas of one row on the GPU: parameters, BatchNorm buffers and counters from the state dict, laid out as the executor says."""

    def __init__(self, lib, h, dev, hw):
        import osi_testlib as T
        sd, x, _ = T.network_case("signed")
        gen = torch.Generator().manual_seed(1011)
        self.x = (x[:B] if hw == HW else torch.rand(B, 3, hw, hw, generator=gen)).contiguous().to(dev)
        self.dlogits = torch.randn(B, C, generator=gen).to(dev)
        self.dfeatures = torch.randn(B, C, generator=gen).to(dev)
        params = torch.zeros(lib.osi_resnet50_param_floats(h))
        buffers = torch.zeros(lib.osi_resnet50_buffer_floats(h))
        nbt = torch.zeros(lib.osi_resnet50_num_bn(h), dtype=torch.int64)
        name = ctypes.create_string_buffer(160)
        off, ne, cc, rm, rv = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        for i in range(lib.osi_resnet50_num_tensors(h)):
            N.check(lib.osi_resnet50_tensor_info(h, i, name, 160, None, None, ctypes.byref(off), ctypes.byref(ne)))
            params[off.value:off.value + ne.value] = sd[name.value.decode()].reshape(-1)
        for j in range(len(nbt)):
            N.check(lib.osi_resnet50_bn_info(h, j, name, 160, ctypes.byref(cc), ctypes.byref(rm), ctypes.byref(rv)))
            pre = name.value.decode()
            buffers[rm.value:rm.value + cc.value] = sd[pre + ".running_mean"]
            buffers[rv.value:rv.value + cc.value] = sd[pre + ".running_var"]
            nbt[j] = int(sd[pre + ".num_batches_tracked"])
        self.params, self.buffers, self.nbt = params.to(dev), buffers.to(dev), nbt.to(dev)
        self.grads = torch.zeros_like(self.params)
        self.ws = torch.zeros(lib.osi_resnet50_workspace_bytes(h), dtype=torch.uint8, device=dev)
        self.logits = torch.zeros(B, C, device=dev)
        self.features = torch.zeros(B, C, device=dev)
        self.dimage = torch.zeros(B, 3, hw, hw, device=dev)
        self.x_adv = torch.zeros(B, hw, hw, 4, device=dev)


def run_row(lib, spec, dev):
    """One row on a fresh executor: (one schedule string per executor call, {name: tensor} of everything the calls wrote)."""
    hw = spec.get("hw", HW)
    knobs = spec.get("knobs", ())
    prev = []
    for k, _ in knobs:
        v = ctypes.c_int()
        N.check(lib.osi_get_tuning(k.encode(), ctypes.byref(v)), k)
        prev.append((k, v.value))
    h = ctypes.c_void_p()
    try:
        for k, v in knobs:      # plan knobs: before the executor exists
            N.check(lib.osi_set_tuning(k.encode(), v), f"{k} = {v}")
        N.check(lib.osi_resnet50_create(ctypes.byref(h), B, hw, hw, C, C, 0), "osi_resnet50_create")
        return _run_calls(lib, h, spec, Case(lib, h, dev, hw))
    finally:
        if h:
            torch.cuda.synchronize()
            lib.osi_resnet50_destroy(h)
        for k, v in reversed(prev):
            N.check(lib.osi_set_tuning(k.encode(), v), k)


def _run_calls(lib, h, spec, c):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, value in spec.get("options", ()):
        N.check(lib.osi_resnet50_set_option(h, name.encode(), value), name)
    if "trainable" in spec:
        N.check(lib.osi_resnet50_set_trainable(h, *spec["trainable"]), "osi_resnet50_set_trainable")
    N.check(lib.osi_resnet50_profile(h, 2))
    cap = 4096
    t, cls, side, n = (ctypes.c_double * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), ctypes.c_int()
    calls = []

    def call(code, what):
        N.check(code, what)
        N.check(lib.osi_resnet50_timeline_read(h, t, cls, side, cap, ctypes.byref(n)), "osi_resnet50_timeline_read")
        assert 0 < n.value < cap and cls[0] == 0
        calls.append("".join(chr(ord("a") + cls[i]) if side[i] else str(cls[i]) for i in range(n.value)))

    P = N.ptr
    fwd = spec.get("fwd", "train")
    if fwd == "frozen":
        call(lib.osi_resnet50_forward_frozen(h, P(c.params), P(c.buffers), P(c.x), P(c.ws), P(c.logits), P(c.features), st), "forward_frozen")
    else:
        call(lib.osi_resnet50_forward(h, P(c.params), P(c.buffers), P(c.nbt), P(c.x), P(c.ws), P(c.logits), P(c.features),
                                      int(fwd == "train"), st), "forward")
    out = dict(logits=c.logits, features=c.features, buffers=c.buffers, nbt=c.nbt)
    bwd = spec.get("bwd", "plain")
    stages = lib.osi_resnet50_num_stages(h)
    common = (h, P(c.params), P(c.grads), P(c.ws), P(c.dlogits), P(c.dfeatures))
    if bwd == "plain" and spec.get("staged"):
        waiter = torch.cuda.Stream()
        for s in range(stages):
            call(lib.osi_resnet50_backward(*common, s, s + 1, st), f"backward stage {s}")
            N.check(lib.osi_resnet50_grads_ready(h, st, ctypes.c_void_p(waiter.cuda_stream)), "osi_resnet50_grads_ready")
        waiter.synchronize()
    elif bwd == "plain":
        call(lib.osi_resnet50_backward(*common, 0, stages, st), "backward")
    elif bwd == "dimage":
        pg = spec["param_grads"]
        call(lib.osi_resnet50_backward_ex(h, P(c.params), P(c.grads) if pg else None, P(c.ws), P(c.dlogits), P(c.dfeatures), P(c.dimage),
                                          pg, 0, stages, st), "backward_ex")
        out["dimage"] = c.dimage
    elif bwd == "adv":
        call(lib.osi_resnet50_backward_adv(*common, P(c.x_adv), 0.01, 0.0, 1.0, 0, stages, st), "backward_adv")
        out["x_adv"] = c.x_adv
    if bwd is not None:
        out["grads"] = c.grads
    N.check(lib.osi_resnet50_profile(h, 0))
    torch.cuda.synchronize()
    return calls, {k: v.cpu() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="hash of the commit the loaded library was built from")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = N.lib()
    rows, blind = {}, []
    for name, spec in ROWS.items():
        calls, _ = run_row(lib, spec, dev)
        print(f"{name}: {len(calls)} calls, {[len(s) for s in calls]} ops")
        if name != "a" and calls == rows["a"]:
            blind.append(name)
        else:
            rows[name] = calls
    doc = {"parent_commit": args.parent, "abi_version_recorded": lib.osi_abi_version(), "geometry": [B, HW, HW, C, C],
           "encoding": "one string per executor call; per op the OSI_PROF class digit on the caller's stream, 'a' + class on the side stream",
           "rows": rows, "blind": blind}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(rows)} rows kept, dropped as blind: {blind or 'none'}")


if __name__ == "__main__":
    main()

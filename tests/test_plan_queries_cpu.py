"""CPU: the host-side launch planners answer what they answered before the planning code was last reworked. tests/golden/plan_queries.json
(tests/golden/make_golden_plans.py, recorded from the library of the commit before) holds the four convolution workspace queries for
every ResNet-50 shape at four batch / image sizes and the workspace of two executors, under the default knobs (tail_cus pinned to 256)
and under one changed knob at a time. A planner that splits differently asks for another slab, so equal numbers mean equal plans."""
import ctypes
import json
import os

import pytest

from openset_imagenet import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_queries.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _follows_256_cus():
    """Without a device the library assumes the MI355X's 256 CUs; what follows the hardware CU count is compared only then, or on such a device."""
    import torch
    return not torch.cuda.is_available() or torch.cuda.get_device_properties(0).multi_processor_count == 256


def _replay(lib, doc, knobs, want, hw_rows):
    prev = []
    try:
        for k, v in knobs:
            old = ctypes.c_int()
            N.check(lib.osi_get_tuning(k.encode(), ctypes.byref(old)), k)
            prev.append((k, old.value))
            N.check(lib.osi_set_tuning(k.encode(), v), f"{k} = {v}")
        compare_hw = _follows_256_cus()
        if not hw_rows or compare_hw:
            for shape, row in zip(doc["shapes"], want["conv"]):
                d = N.ConvDesc.make(*shape)
                got = [None if w is None else getattr(lib, q)(ctypes.byref(d)) for q, w in zip(doc["queries"], row)]
                assert got == row, (knobs, shape, doc["queries"], got, row)
        if compare_hw:         # the stem's weight-gradient grid and the backward Winograd plans follow the hardware CU count
            for args, bytes_ in zip(doc["executor_args"], want["executors"]):
                h = ctypes.c_void_p()
                N.check(lib.osi_resnet50_create(ctypes.byref(h), *args, 0), "osi_resnet50_create")
                try:
                    assert lib.osi_resnet50_workspace_bytes(h) == bytes_, (knobs, args)
                finally:
                    lib.osi_resnet50_destroy(h)
    finally:
        for k, v in reversed(prev):
            N.check(lib.osi_set_tuning(k.encode(), v), k)


def test_fixture_has_no_blind_row(golden):
    base = golden["defaults"]
    assert len(golden["shapes"]) >= 80 and len(golden["settings"]) >= 10
    for s in golden["settings"]:
        assert s["conv"] != base["conv"] or s["executors"] != base["executors"], (s["knob"], s["value"])


def test_plans_under_the_default_knobs(golden):
    _replay(N.lib(), golden, [tuple(golden["pin"])], golden["defaults"], hw_rows=False)


def test_plans_under_one_changed_knob_at_a_time(golden):
    lib, pin = N.lib(), tuple(golden["pin"])
    for s in golden["settings"]:
        one = (s["knob"], s["value"])
        knobs = [one] if one[0] == pin[0] or not s["pinned"] else [pin, one]
        _replay(lib, golden, knobs, s, hw_rows=not s["pinned"])

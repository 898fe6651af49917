"""GPU: the whole-network executor enqueues what it enqueued before csrc/resnet50_exec.hip was last reworked. tests/golden/exec_schedule.json
(tests/golden/make_golden_schedule.py, recorded from the library of the commit before) holds, per executor call, the class and the
stream of every op in issue order, read back through the executor's own timeline instrumentation, for every route the executor has:
training / frozen / inference forwards, one-call and staged backwards, the image-gradient and adversarial requests, fine-tuning cuts
with and without an inference-form prefix, the side stream off, the Winograd forms off, and a geometry that takes the materialised stem
tail. Only the times vary between runs; the (class, stream) pairs are deterministic, so the comparison is exact.
It does not see event waits or scratch-buffer identities. Each row builds one B = 2 executor at 64 x 64 (72 x 72) and runs one step."""
import importlib.util
import json
import os

import pytest
import torch

from openset_imagenet import _native as N

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN_DIR, "exec_schedule.json")) as _f:
    GOLDEN = json.load(_f)


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_schedule", os.path.join(GOLDEN_DIR, "make_golden_schedule.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_rows_and_has_no_blind_one():
    M = _recorder()
    rows, blind = GOLDEN["rows"], GOLDEN["blind"]
    assert sorted(list(rows) + blind) == sorted(M.ROWS) and "a" in rows
    assert GOLDEN["geometry"] == [M.B, M.HW, M.HW, M.C, M.C] and len(GOLDEN["parent_commit"]) >= 7
    for name, calls in rows.items():
        assert name == "a" or calls != rows["a"], name
        assert all(c[0] == "0" for c in calls), name       # every executor call opens with the start mark on the caller's stream
    assert len(rows["e"]) == 5 and len(rows["g"]) == 1      # call boundaries are part of the record: forward + four stages; forward only
    assert any(ch.isalpha() for ch in rows["a"][1]) and not any(ch.isalpha() for c in rows["b"] for ch in c)   # side stream on / off


@pytest.mark.parametrize("row", sorted(GOLDEN["rows"]))
def test_executor_schedule_matches_the_recording(cuda, row):
    M = _recorder()
    calls, outs = M.run_row(N.lib(), M.ROWS[row], cuda)
    want = GOLDEN["rows"][row]
    assert len(calls) == len(want), f"row {row}: {len(calls)} executor calls, {len(want)} recorded"
    for i, (got, exp) in enumerate(zip(calls, want)):
        if got != exp:
            at = next((j for j, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
            pytest.fail(f"row {row}, call {i}: {len(got)} ops against {len(exp)} recorded, first difference at op {at}: "
                        f"...{got[max(0, at - 8):at + 8]} against ...{exp[max(0, at - 8):at + 8]}")
    assert all(bool(torch.isfinite(v.double()).all()) for v in outs.values()), f"row {row}: a non-finite output"

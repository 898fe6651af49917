"""GPU: the BatchNorm entry points of csrc/bn.hip write the bits they wrote before the file's host half and its partial-sum walkers were
last reworked. tests/golden/bn_digests.json (tests/golden/make_golden_bn_digests.py, recorded from the library of the commit before)
holds, per kernel form, a SHA-256 of every buffer the call writes, the workspace included: statistics with and without running
statistics; the three finalisers of [P][C] partials (256-thread, 1024-thread, two-level) at partial counts that run their unrolled loops,
their tails and the clamped channel lanes; the forward apply in its four residual / ReLU settings, with the ReLU bitmask and with the
fused shortcut; the backward plain, gated by the activation or the bitmask, emitting g and in place; the stem tail's pool-gather
backward and its frozen twin; the fused backward and the bare reduction on seeded partials through the one-launch and the two-level
reducers; the two-consumer backward on even, odd and uncapped grids; the frozen backward in all its settings. Streamed shapes take every
channel geometry of the streaming passes (C = 64, 96, 2048, and 2048 under a grid of 7). Inputs are CPU-seeded, buffers NaN-prefilled and
digested whole, the four BatchNorm knobs pinned per case and restored; each case is one to three launches of at most 37 x 2048 elements."""
import importlib.util
import json
import os

import pytest

from openset_imagenet import _native as N

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN_DIR, "bn_digests.json")) as _f:
    GOLDEN = json.load(_f)


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_bn_digests", os.path.join(GOLDEN_DIR, "make_golden_bn_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _recorder()


def _expected_outputs(c):
    """What a case must have a digest of, from the case's description alone (not from what the recorder happened to return)."""
    fn = c["fn"]
    per_channel = {"mean", "invstd", "scale", "shift"}
    if fn == "stats":
        return per_channel | {"ws"} | ({"running_mean", "running_var"} if c["running"] else set())
    if fn == "final":
        return per_channel | {"ws", "running_mean", "running_var"}
    if fn == "apply":
        return {"out"}
    if fn in ("apply_mask", "apply_mask2"):
        return {"out", "mask"}
    sums = {"dgamma", "dbeta", "ws"}
    if fn in ("bwd", "bwd_mask"):
        return sums | {"dy"} | ({"gmasked"} if c["gm"] else set())
    if fn == "fused":
        return sums | {"dy"}
    if fn == "reduce":
        return sums
    if fn == "fused2":
        return {"ws"} | {f"{k}{i}" for k in ("dy", "dgamma", "dbeta") for i in (0, 1)}
    if fn == "frozen":
        want = {f"dy{i}" for i in range(c["n"])} | ({"gmasked"} if c["gm"] else set())
        return want | ({"ws"} | {f"{k}{i}" for k in ("dgamma", "dbeta") for i in range(c["n"])} if c["pgrad"] else set())
    assert fn == "pool", fn
    return ({"dy"} if c["dy"] else set()) | (sums if c["pgrad"] else set())


def test_fixture_covers_the_cases_and_names_their_outputs():
    assert sorted(GOLDEN["cases"]) == sorted(M.CASES)
    assert len(GOLDEN["parent_commit"]) >= 7 and GOLDEN["date"] and GOLDEN["recorded_on"]
    for name, c in M.CASES.items():
        assert set(GOLDEN["cases"][name]) == _expected_outputs(c) == set(M.outputs_of(c)), name
        assert all(len(v) == 64 for v in GOLDEN["cases"][name].values()), name
        assert set(c["knobs"]) <= set(M.KNOBS), name
    # forms that share their inputs and must differ, and forms that must not: spot checks that the digests tell forms apart
    g = GOLDEN["cases"]
    assert g["apply_37x96_res0_relu0"]["out"] != g["apply_37x96_res0_relu1"]["out"] != g["apply_37x96_res1_relu1"]["out"]
    assert g["apply_mask_37x96_res1"]["out"] == g["apply_37x96_res1_relu1"]["out"], "the bitmask form writes the ReLU output of the plain form"
    assert g["bwd_37x96_act0_gm0"]["dy"] != g["bwd_37x96_act1_gm0"]["dy"] == g["bwd_37x96_act1_inplace"]["dy"]
    assert g["apply_37x2048_res1_relu1"] == g["apply_37x2048_grid7_res1_relu1"], "element-wise: the grid does not change the bits"
    assert g["fused2_37x2048_grid7"] == g["fused2_37x2048_grid8"], "per-element and per-lane coefficients: the same bits"
    assert g["fused_37x96_P200"]["dgamma"] != g["fused_37x96_P257"]["dgamma"]


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_batchnorm_outputs_match_the_recorded_digests(cuda, name):
    assert name in GOLDEN["cases"], f"{name}: not in the fixture"
    got = M.run_case(N.lib(), name, cuda)
    print(name, got)
    assert got == GOLDEN["cases"][name], name

"""GPU: the forward and input-gradient convolutions of csrc/conv_igemm.hip write the bits they wrote before their exit paths were
last reworked. tests/golden/conv_exit_digests.json (tests/golden/make_golden_conv_digests.py, recorded from the library of the commit
before) holds, per kernel form, a SHA-256 of every output: y / dx and the used part of the BatchNorm statistics / partial-sum
workspace. Forms: the 64x64 tile plain / with the fused input activation / with a fused shortcut, row windows, other tile ids (scalar
epilogue), the row walker, the K-split tail + fix-up pass with statistics and with the inference epilogue, the inference epilogue in
its three settings on two tiles, and the input gradient plain and in its four fused flavours, on row windows, at stride 2 and with a
K-split tail. Inputs are CPU-seeded, outputs NaN-prefilled, every shape has a ragged last row tile, every plan knob is pinned and
restored; each case is one or two launches of a few hundred pixels."""
import importlib.util
import json
import os

import pytest

from openset_imagenet import _native as N

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN_DIR, "conv_exit_digests.json")) as _f:
    GOLDEN = json.load(_f)


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_conv_digests", os.path.join(GOLDEN_DIR, "make_golden_conv_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _recorder()


def test_fixture_covers_the_cases_and_has_no_blind_one():
    assert sorted(GOLDEN["cases"]) == sorted(M.CASES) and GOLDEN["blind"] == []
    assert len(GOLDEN["parent_commit"]) >= 7 and GOLDEN["recorded_on"]
    for name, c in M.CASES.items():
        if c["dir"] == "dgrad":
            want = {"dx"} if c["flavour"] == 0 else {"dx", "sums", "partials"}
        else:
            want = {"y"} if c["form"] in M.EPI else {"y", "stats", "partials"}
        assert set(GOLDEN["cases"][name]) == want, name
        assert all(len(v) == 64 for k, v in GOLDEN["cases"][name].items() if k != "partials"), name
    # the cases that exist for a knob are told apart from their knob-off form by the recording itself; spot-check two pairs of forms
    # that share inputs and must differ
    g = GOLDEN["cases"]
    assert g["fwd_epi_relu_64x64"]["y"] != g["fwd_epi_raw_64x64"]["y"] != g["fwd_epi_res_relu_64x64"]["y"]
    assert g["dgrad_3x3_fl2"]["dx"] != g["dgrad_3x3_w3_fl2"]["dx"] and g["dgrad_3x3_fl2"]["dx"] != g["dgrad_3x3_fl4"]["dx"]


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_convolution_outputs_match_the_recorded_digests(cuda, name):
    assert name in GOLDEN["cases"], f"{name}: not in the fixture (blind: {GOLDEN['blind']})"
    got = M.run_case(N.lib(), name, cuda)
    print(name, got)
    assert got == GOLDEN["cases"][name], name
    twin = M.CASES[name]["twin"]
    if twin is not None:      # the row walker reproduces the tile kernel bit for bit
        assert M.run_case(N.lib(), name, cuda, twin) == got, f"{name}: differs from the launch with {twin}"

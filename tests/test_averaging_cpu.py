"""CPU: weight averaging (EMA / SWA, ABI 20) without a GPU — the exported symbols, every argument refusal of osi_average_update and
osi_resnet50_set_bn_momentum (nothing is launched), AveragedModel on a plain torch module bit for bit against
torch.optim.swa_utils.AveragedModel, the state-dict schema of an averaged ResNet50, the `avg` config block, and the checkpoint keys."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn
from torch.optim import swa_utils

from openset_imagenet import _native as N

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("osi_average_update", "osi_resnet50_set_bn_momentum", "osi_resnet50_get_bn_momentum")


def test_new_symbols_are_exported_declared_and_bound():
    lib = N.lib()
    header = open(os.path.join(ROOT, "include", "osi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/osi.h"
        assert name in N.declared_symbols(), f"{name} is missing from the ctypes table"
    assert "OSI_AVG_MAX_SPANS 4" in header and N.AVG_MAX_SPANS == 4
    assert lib.osi_abi_version() >= 20


# ---- osi_average_update: every refusal comes before any launch ----------------------------------------------------------------------
A, C, A2, C2 = 0x10000, 0x20000, 0x30000, 0x40000     # 16-byte aligned addresses that are never dereferenced


def _call(spans, weight=0.5, n_spans=None):
    table = (N.AvgSpan * max(len(spans), 1))(*[N.AvgSpan(a, c, n) for a, c, n in spans])
    return N.lib().osi_average_update(table, len(spans) if n_spans is None else n_spans, weight, None)


def test_average_update_refuses_a_null_table():
    assert N.lib().osi_average_update(None, 1, 0.5, None) == -1


@pytest.mark.parametrize("n_spans", [0, -1, 5])
def test_average_update_refuses_a_span_count_outside_1_to_4(n_spans):
    assert _call([(A, C, 16)] * 5, n_spans=n_spans) == -1


def test_average_update_refuses_a_null_pointer():
    assert _call([(None, C, 16)]) == -1
    assert _call([(A, None, 16)]) == -1
    assert _call([(A, C, 16), (A2, None, 16)]) == -1


def test_average_update_refuses_a_misaligned_pointer():
    assert _call([(A + 4, C, 16)]) == -1
    assert _call([(A, C + 8, 16)]) == -1


def test_average_update_refuses_an_empty_span():
    assert _call([(A, C, 0)]) == -1


def test_average_update_refuses_a_length_that_is_no_multiple_of_four():
    assert _call([(A, C, 18)]) == -1


def test_average_update_refuses_more_units_than_32_bit_indices_hold():
    big = 4 * (2 ** 32 - 511)                          # n / 4 = 2^32 - 511 > 2^32 - 512
    assert _call([(1 << 40, 1 << 44, big)]) == -1


@pytest.mark.parametrize("weight", [float("nan"), -0.25, 1.5, float("inf"), -0.0 - 1e-30])
def test_average_update_refuses_a_weight_outside_0_to_1(weight):
    assert _call([(A, C, 16)], weight=weight) == -1


def test_average_update_refuses_an_average_that_overlaps_a_current_range():
    assert _call([(A, A, 16)]) == -1                               # its own
    assert _call([(A, A + 32, 16)]) == -1                          # 16 floats = 64 bytes: [A, A + 64) meets [A + 32, A + 96)
    assert _call([(A, C, 16), (A2, A + 48, 16)]) == -1             # another span's


def test_average_update_refuses_two_averages_that_overlap():
    assert _call([(A, C, 16), (A + 16, C2, 16)]) == -1
    assert _call([(A, C, 16), (A, C2, 16)]) == -1


# ---- the executor's BatchNorm momentum ----------------------------------------------------------------------------------------------
def test_bn_momentum_setter_refuses_and_getter_reports():
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(h), 4, 32, 32, 8, 8, 0) == 0
    try:
        m = ctypes.c_float(-1.0)
        assert lib.osi_resnet50_get_bn_momentum(h, ctypes.byref(m)) == 0 and m.value == ctypes.c_float(0.1).value
        for bad in (0.0, -0.1, 1.5, float("nan")):
            assert lib.osi_resnet50_set_bn_momentum(h, bad) == -1, bad
            assert lib.osi_resnet50_get_bn_momentum(h, ctypes.byref(m)) == 0 and m.value == ctypes.c_float(0.1).value
        for good in (1.0, 1.0 / 3.0, 0.1):
            assert lib.osi_resnet50_set_bn_momentum(h, good) == 0
            assert lib.osi_resnet50_get_bn_momentum(h, ctypes.byref(m)) == 0 and m.value == ctypes.c_float(good).value
        assert lib.osi_resnet50_set_bn_momentum(None, 0.5) == -1 and lib.osi_resnet50_get_bn_momentum(h, None) == -1
    finally:
        lib.osi_resnet50_destroy(h)


def test_model_bn_momentum_property_checks_its_range():
    from openset_imagenet import ResNet50
    model = ResNet50(8, 8, False)
    assert model.bn_momentum == 0.1
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            model.bn_momentum = bad
    model.bn_momentum = 0.25                           # no executor exists yet: the value waits for the ones the model creates
    assert model.bn_momentum == 0.25


# ---- AveragedModel on a plain torch module against torch.optim.swa_utils ----------------------------------------------------------
class Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 5, 3)
        self.bn = nn.BatchNorm2d(5)
        self.fc = nn.Linear(5, 4)

    def forward(self, x):
        return self.fc(self.bn(self.conv(x)).mean((2, 3)))


@pytest.mark.parametrize("buffers", ["copy", "average"])
@pytest.mark.parametrize("kind", ["ema", "swa"])
def test_plain_module_is_bit_equal_to_swa_utils(kind, buffers):
    from openset_imagenet.averaging import AveragedModel
    torch.manual_seed(3)
    model = Small()
    decay = 0.9
    fn = swa_utils.get_ema_multi_avg_fn(decay) if kind == "ema" else swa_utils.get_swa_multi_avg_fn()
    if kind == "swa" and buffers == "average":
        # torch's own swa_update raises on the int64 group that use_buffers=True hands it (num_batches_tracked: "Integer division with
        # addcdiv is no longer supported"); the floating-point groups go through torch's function unchanged, the counter is left alone
        swa = fn
        fn = lambda avg, cur, n: swa(avg, cur, n) if avg[0].is_floating_point() else None
    ref = swa_utils.AveragedModel(model, multi_avg_fn=fn, use_buffers=buffers == "average")
    ours = AveragedModel(model, kind=kind, decay=decay, buffers=buffers)
    assert ours.module is not model and not any(a is b for a, b in zip(ours.module.parameters(), model.parameters()))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    gen = torch.Generator().manual_seed(4)
    for step in range(5):
        model.train()
        opt.zero_grad()
        model(torch.randn(6, 3, 8, 8, generator=gen)).square().sum().backward()
        opt.step()
        ref.update_parameters(model)
        ours.update_parameters(model)
        assert int(ours.n_averaged) == int(ref.n_averaged) == step + 1
        mine, theirs = ours.state_dict(), ref.state_dict()
        assert list(mine) == list(theirs)
        for key, value in theirs.items():
            if value.is_floating_point():
                assert torch.equal(mine[key].view(torch.int32), value.view(torch.int32)), (step, key)
    # the counter of the BatchNorm is copied (torch's integer "average" under use_buffers=True is not reproduced)
    assert int(ours.module.bn.num_batches_tracked) == int(model.bn.num_batches_tracked) == 5
    # the averages moved, and are not the model
    assert not torch.equal(ours.module.fc.weight, model.fc.weight)


# ---- the state-dict schema of an averaged ResNet50 ---------------------------------------------------------------------------------
def test_resnet50_state_dict_is_swa_utils_schema_and_loads_both_ways():
    from openset_imagenet import ResNet50
    from openset_imagenet.averaging import AveragedModel
    torch.manual_seed(5)
    model = ResNet50(8, 8, False)
    ours = AveragedModel(model)
    assert isinstance(ours.module, ResNet50) and ours.module is not model
    assert ours.module._flat_params.data_ptr() != model._flat_params.data_ptr()          # arenas of its own, filled from the model's
    assert torch.equal(ours.module._flat_params, model._flat_params) and torch.equal(ours.module._flat_buffers, model._flat_buffers)
    p0 = ours.module._plist[0]
    assert p0.data_ptr() == ours.module._flat_params.data_ptr() + 4 * ours.module._pinfo[0][1]   # still views into ONE arena
    theirs = swa_utils.AveragedModel(ResNet50(8, 8, False))
    assert list(ours.state_dict()) == list(theirs.state_dict())
    assert list(ours.state_dict())[0] == "n_averaged" and "module.resnet_base.conv1.weight" in ours.state_dict()
    # ours -> torch's
    with torch.no_grad():
        ours.module._flat_params.mul_(1.5)
        ours.module._flat_buffers.add_(0.25)
    ours.n_averaged.fill_(7)
    theirs.load_state_dict(ours.state_dict())
    assert int(theirs.n_averaged) == 7
    for key, value in ours.state_dict().items():
        assert torch.equal(theirs.state_dict()[key], value), key
    # torch's -> ours
    other = swa_utils.AveragedModel(ResNet50(8, 8, False))
    other.n_averaged.fill_(11)
    back = AveragedModel(model, kind="swa")
    back.load_state_dict(other.state_dict())
    assert int(back.n_averaged) == 11 and back._n == 11
    for key, value in other.state_dict().items():
        assert torch.equal(back.state_dict()[key], value), key


# ---- the config block -----------------------------------------------------------------------------------------------------------------
def _cfg(block):
    from openset_imagenet.util import NameSpace
    return NameSpace({"avg": block} if block is not None else {})


def test_config_absent_or_off_is_none_and_defaults_hold():
    from openset_imagenet.averaging import options
    assert options(_cfg(None)) is None
    assert options(_cfg({"kind": "off"})) is None
    assert options(_cfg({"kind": False})) is None               # YAML reads a bare `off` as False
    assert options(_cfg({"kind": "off", "decay": 0.5, "every": 3})) is None
    o = options(_cfg({"kind": "ema"}))
    assert (o.kind, o.decay, o.every, o.start_epoch, o.buffers, o.select, o.update_bn) == ("ema", 0.9998, 1, 0, "copy", "model", False)
    o = options(_cfg({"kind": "swa", "every": 4, "start_epoch": 90, "buffers": "average", "select": "averaged", "update_bn": "on"}))
    assert (o.kind, o.every, o.start_epoch, o.buffers, o.select, o.update_bn) == ("swa", 4, 90, "average", "averaged", True)


@pytest.mark.parametrize("block", [
    {"kind": "mean"}, {"kind": 3}, {"kind": "ema", "decay": 1.5}, {"kind": "ema", "decay": -0.1}, {"kind": "ema", "decay": "high"},
    {"kind": "ema", "decay": float("nan")}, {"kind": "ema", "decay": True}, {"kind": "ema", "every": 0}, {"kind": "ema", "every": 1.5},
    {"kind": "ema", "every": True}, {"kind": "ema", "every": "2"}, {"kind": "swa", "start_epoch": -1}, {"kind": "swa", "start_epoch": 0.5},
    {"kind": "ema", "buffers": "mean"}, {"kind": "ema", "buffers": True}, {"kind": "ema", "select": "best"}, {"kind": "ema", "select": 1},
    {"kind": "ema", "update_bn": "maybe"}, {"kind": "ema", "update_bn": 2}, {"kind": "ema", "momentum": 0.9}, {"kind": "off", "every": 0},
    "ema", 3])
def test_config_refuses_malformed_values(block):
    from openset_imagenet.averaging import options
    with pytest.raises(ValueError):
        options(_cfg(block))


def test_constructor_refuses_malformed_arguments():
    from openset_imagenet.averaging import AveragedModel
    for kw in ({"kind": "mean"}, {"buffers": "mean"}, {"decay": 1.5}, {"decay": float("nan")}):
        with pytest.raises(ValueError):
            AveragedModel(Small(), **kw)


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------------
def test_save_checkpoint_without_an_average_writes_todays_keys(tmp_path):
    from openset_imagenet.averaging import AveragedModel
    from openset_imagenet.train import load_checkpoint, save_checkpoint
    from openset_imagenet import tools
    tools.set_device_cpu()
    torch.manual_seed(6)
    model = Small()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1)
    save_checkpoint(tmp_path / "plain.pth", model, 3, opt, 0.5)
    assert sorted(torch.load(tmp_path / "plain.pth", weights_only=False)) == ["best_score", "epoch", "model_state_dict", "opt_state_dict"]
    save_checkpoint(tmp_path / "sched.pth", model, 3, opt, 0.5, sched)
    assert sorted(torch.load(tmp_path / "sched.pth", weights_only=False)) == ["best_score", "epoch", "model_state_dict", "opt_state_dict", "scheduler"]
    averaged = AveragedModel(model, kind="swa")
    averaged.update_parameters(model)
    with torch.no_grad():
        model.fc.weight.add_(1.0)
    averaged.update_parameters(model)
    save_checkpoint(tmp_path / "avg.pth", model, 3, opt, 0.5, averaged=averaged)
    data = torch.load(tmp_path / "avg.pth", weights_only=False)
    assert sorted(data) == ["avg_state_dict", "best_score", "epoch", "model_state_dict", "opt_state_dict"]
    assert int(data["avg_state_dict"]["n_averaged"]) == 2
    # restored; and a checkpoint without the key restarts the average from the loaded weights
    again = AveragedModel(Small(), kind="swa")
    assert load_checkpoint(Small(), tmp_path / "avg.pth", averaged=again) == (4, 0.5)
    assert again._n == 2 and torch.equal(again.module.fc.weight, averaged.module.fc.weight)
    target = Small()
    load_checkpoint(target, tmp_path / "plain.pth", averaged=again)
    assert again._n == 0 and int(again.n_averaged) == 0 and torch.equal(again.module.fc.weight, target.fc.weight)


def test_evaluate_averaged_takes_the_checkpoints_module_or_exits(tmp_path):
    from openset_imagenet import ResNet50
    from openset_imagenet.averaging import AveragedModel
    from openset_imagenet.script.evaluate import averaged_module, get_args
    from openset_imagenet.train import save_checkpoint
    assert get_args(["entropic", "2", "--averaged"]).averaged and not get_args(["entropic", "2"]).averaged
    torch.manual_seed(8)
    model = ResNet50(8, 8, False)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    save_checkpoint(tmp_path / "plain.pth", model, 0, opt, 0.0)
    with pytest.raises(SystemExit, match="avg_state_dict"):
        averaged_module(ResNet50(8, 8, False), tmp_path / "plain.pth")
    averaged = AveragedModel(model)
    with torch.no_grad():
        averaged.module._flat_params.mul_(0.5)
    save_checkpoint(tmp_path / "avg.pth", model, 0, opt, 0.0, averaged=averaged)
    module = averaged_module(ResNet50(8, 8, False), tmp_path / "avg.pth")
    assert isinstance(module, ResNet50) and torch.equal(module._flat_params, averaged.module._flat_params)
    assert not torch.equal(module._flat_params, model._flat_params)

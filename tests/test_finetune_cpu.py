"""CPU: fine-tuning a suffix (ABI 13) — the five unit / trainable entry points, the unit table against the state-dict names, the
argument rules of osi_resnet50_set_trainable, and the host logic of ResNet50.freeze_below, the mask derived from requires_grad, the
config key and the fgsm refusal. Nothing here launches a kernel."""
import ctypes
import os
import re

import pytest

from openset_imagenet import _native as N

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = ("osi_resnet50_num_units", "osi_resnet50_tensor_unit", "osi_resnet50_bn_unit", "osi_resnet50_set_trainable",
       "osi_resnet50_get_trainable")
ERR_ARG, ERR_STATE = -1, -3
FULL = 0x3FFFF
BLOCKS = (3, 4, 6, 3)


def unit_of_name(name):
    """Unit of a state-dict key / BatchNorm prefix, from the NAME (the table under test comes from the executor's construction)."""
    parts = name.split(".")
    if parts[0] == "logits" or parts[1] == "fc":
        return 17
    if parts[1] in ("conv1", "bn1"):
        return 0
    layer, block = int(parts[1][len("layer"):]), int(parts[2])
    return 1 + sum(BLOCKS[:layer - 1]) + block


def test_unit_symbols_declared_exported_and_bound():
    lib = N.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "osi.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in include/osi.h"
        assert hasattr(lib, s), f"{s} is not exported by libosi_hip.so"
        assert s in N.declared_symbols(), f"{s} is missing from the ctypes table"
    assert lib.osi_abi_version() >= 13


@pytest.fixture()
def net():
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(h), 2, 64, 64, 10, 10, 0) == 0
    yield h
    lib.osi_resnet50_destroy(h)


def test_unit_table_matches_the_state_dict_names(net):
    lib = N.lib()
    assert lib.osi_resnet50_num_units(net) == 18
    name = ctypes.create_string_buffer(160)
    nt, nb = lib.osi_resnet50_num_tensors(net), lib.osi_resnet50_num_bn(net)
    assert (nt, nb) == (162, 53)             # 53 convolutions, 106 BatchNorm affine tensors, fc weight and bias, logits weight
    seen = set()
    for i in range(nt):
        assert lib.osi_resnet50_tensor_info(net, i, name, 160, None, None, None, None) == 0
        assert lib.osi_resnet50_tensor_unit(net, i) == unit_of_name(name.value.decode()), name.value
        seen.add(lib.osi_resnet50_tensor_unit(net, i))
    assert seen == set(range(18))
    units = []
    for j in range(nb):
        assert lib.osi_resnet50_bn_info(net, j, name, 160, None, None, None) == 0
        assert lib.osi_resnet50_bn_unit(net, j) == unit_of_name(name.value.decode()), name.value
        units.append(lib.osi_resnet50_bn_unit(net, j))
    assert units == sorted(units)                    # forward order: the BatchNorms of a suffix are a tail of the table
    for bad in (-1, nt, 10 ** 6):
        assert lib.osi_resnet50_tensor_unit(net, bad) == -1
    for bad in (-1, nb, 10 ** 6):
        assert lib.osi_resnet50_bn_unit(net, bad) == -1
    assert lib.osi_resnet50_tensor_unit(None, 0) == -1 and lib.osi_resnet50_bn_unit(None, 0) == -1


def test_set_trainable_round_trip_and_argument_rules(net):
    lib = N.lib()
    mask, p = ctypes.c_uint(7), ctypes.c_int(-5)

    def get():
        assert lib.osi_resnet50_get_trainable(net, ctypes.byref(mask), ctypes.byref(p)) == 0
        return mask.value, p.value

    assert get() == (FULL, 0)
    for m, q in ((0x3E000, 13), (0x3E000, 0), (0x20000, 17), (0x3FFE1, 0), (0x3FFFE, 1), (FULL, 0)):
        assert lib.osi_resnet50_set_trainable(net, m, q) == 0
        assert get() == (m, q)
    assert lib.osi_resnet50_set_trainable(net, 0x3E000, 5) == 0
    for m, q in ((0, 0), (1 << 18, 0), (FULL | (1 << 18), 0), (0x3E000, 14), (FULL, 1), (0x3E000, -1), (0x20000, 18)):
        assert lib.osi_resnet50_set_trainable(net, m, q) == ERR_ARG, (hex(m), q)
        assert get() == (0x3E000, 5)                 # a refused call changes nothing
    assert lib.osi_resnet50_set_trainable(None, FULL, 0) == ERR_ARG
    assert lib.osi_resnet50_get_trainable(net, None, ctypes.byref(p)) == ERR_ARG


# ---- host logic of the Python layer --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from openset_imagenet import ResNet50
    return ResNet50(10, 10, False)


def flags(m):
    return {n: p.requires_grad for n, p in m.named_parameters()}


def test_freeze_below_names_flags_and_property(model):
    m = model
    names = [n for n, _ in m.named_parameters()]
    assert m.frozen_below is None
    for bad in ("layer0", "layer5", "layer1.3", "layer3.6", "stem", "conv1", "logits", "layer4.", "", 4, "LAYER4", "fc.weight"):
        with pytest.raises(ValueError):
            m.freeze_below(bad)
    assert m.frozen_below is None and all(flags(m).values())
    with pytest.raises(AttributeError):
        m.frozen_below = "fc"

    assert m.freeze_below("layer4") is m and m.frozen_below == "layer4.0"
    assert flags(m) == {n: unit_of_name(n) >= 14 for n in names}
    m.freeze_below("layer3.2")                       # moving the cut down gives back what the earlier call froze
    assert m.frozen_below == "layer3.2" and flags(m) == {n: unit_of_name(n) >= 10 for n in names}
    m.freeze_below("fc")
    assert m.frozen_below == "fc" and flags(m) == {n: unit_of_name(n) == 17 for n in names}
    m.freeze_below("layer1")                         # stem only
    assert m.frozen_below == "layer1.0" and flags(m) == {n: unit_of_name(n) >= 1 for n in names}
    m.freeze_below(None)
    assert m.frozen_below is None and all(flags(m).values())

    # flags somebody else set are never touched: neither turned on by a cut that moves, nor by clearing it
    byhand = "resnet_base.layer4.1.conv2.weight"
    dict(m.named_parameters())[byhand].requires_grad_(False)
    dict(m.named_parameters())["resnet_base.layer1.0.bn1.bias"].requires_grad_(False)
    m.freeze_below("layer2")
    m.freeze_below("layer1.1")
    assert not flags(m)[byhand] and not flags(m)["resnet_base.layer1.0.bn1.bias"]
    m.freeze_below(None)
    assert [n for n, f in flags(m).items() if not f] == ["resnet_base.layer1.0.bn1.bias", byhand]
    for p in m.parameters():
        p.requires_grad_(True)


def test_unit_mask_from_requires_grad(model):
    m = model
    assert m._trainable_plan() == (FULL, (True, True, True, True))
    for n, p in m.named_parameters():                # layer1 (units 1 - 3) frozen under a trainable stem: the cut stays at unit 0
        p.requires_grad_(not n.startswith("resnet_base.layer1."))
    mask, live = m._trainable_plan()
    assert mask == 0x3FFF1 and (mask & -mask) == 1 and live == (True, True, True, True)
    for n, p in m.named_parameters():                # head only: one bit, only backward stage 0 holds a trainable tensor
        p.requires_grad_(unit_of_name(n) == 17)
    assert m._trainable_plan() == (0x20000, (True, False, False, False))
    for n, p in m.named_parameters():                # one BatchNorm bias of layer2.1 keeps its unit trainable
        p.requires_grad_(n == "resnet_base.layer2.1.bn2.bias")
    assert m._trainable_plan() == (1 << 5, (False, False, True, False))
    for p in m.parameters():
        p.requires_grad_(False)
    assert m._trainable_plan() == (0, (False, False, False, False))
    for p in m.parameters():
        p.requires_grad_(True)
    m.freeze_below("layer3")
    assert m._trainable_plan() == (0x3FF00, (True, True, False, False))
    m.freeze_below(None)
    assert m._trainable_plan()[0] == FULL


def test_config_key_and_fgsm_refusal():
    from openset_imagenet import adversary as A
    from openset_imagenet import train as T

    class Cfg:
        pass
    cfg = Cfg()
    assert T._freeze_below_of(cfg) is None           # absent = off
    for value, want in ((None, None), (False, None), ("off", None), ("layer4", "layer4"), ("layer3.2", "layer3.2"), ("fc", "fc")):
        cfg.freeze_below = value
        assert T._freeze_below_of(cfg) == want
    for value in (4, True, ["layer4"]):
        cfg.freeze_below = value
        with pytest.raises(ValueError):
            T._freeze_below_of(cfg)

    cfg.loss, cfg.adv = Cfg(), Cfg()
    cfg.loss.type, cfg.adv.epsilon, cfg.adv.std = "entropic", 0.1, 0.1
    cfg.freeze_below = "layer4"
    cfg.adv.who = "fgsm"
    with pytest.raises(ValueError, match="freeze_below"):
        A.Plan(cfg)
    for who in ("gaussian", "uniform"):              # the noise modes need no image gradient
        cfg.adv.who = who
        assert A.Plan(cfg).who == who
    cfg.freeze_below, cfg.adv.who = None, "fgsm"
    assert A.Plan(cfg).who == "fgsm"

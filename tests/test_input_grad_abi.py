"""CPU: the input-gradient entry points of ABI 8 (osi_stem_dgrad, osi_resnet50_backward_ex) are exported, declared in the ctypes
table, and refuse bad arguments with OSI_ERR_ARG before anything is launched (safe on a host without a GPU)."""
import ctypes

import pytest

from openset_imagenet import _native as N

ERR_ARG, ERR_STATE = -1, -3


def test_symbols_exported_and_abi_version():
    lib = N.lib()
    for s in ("osi_stem_dgrad", "osi_resnet50_backward_ex"):
        assert hasattr(lib, s), s
        assert s in N.declared_symbols(), s
    assert lib.osi_abi_version() >= 8


def test_stem_dgrad_argument_errors():
    lib = N.lib()
    dy, w, dx = 1 << 20, 1 << 21, 1 << 22          # aligned fake addresses: nothing may be launched, so nothing is dereferenced
    assert lib.osi_stem_dgrad(None, w, dx, 2, 64, 64, None) == ERR_ARG
    assert lib.osi_stem_dgrad(dy, None, dx, 2, 64, 64, None) == ERR_ARG
    assert lib.osi_stem_dgrad(dy, w, None, 2, 64, 64, None) == ERR_ARG
    assert lib.osi_stem_dgrad(dy, w, dx, 0, 64, 64, None) == ERR_ARG            # empty batch
    assert lib.osi_stem_dgrad(dy, w, dx, 2, 31, 64, None) == ERR_ARG            # below the executor's smallest image
    assert lib.osi_stem_dgrad(dy, w, dx, 2, 64, 16, None) == ERR_ARG
    assert lib.osi_stem_dgrad(dy + 4, w, dx, 2, 64, 64, None) == ERR_ARG        # dY is read in 16-byte vectors
    assert lib.osi_stem_dgrad(dy, w, dx + 2, 2, 64, 64, None) == ERR_ARG        # misaligned output
    assert lib.osi_stem_dgrad(dy, w, dx, 4096, 224, 224, None) == ERR_ARG       # dY beyond 32-bit buffer offsets (4096 x 112^2 x 64 x 4 B)


@pytest.fixture
def net():
    lib = N.lib()
    h = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(h), 2, 64, 64, 16, 16, 0) == 0
    yield h
    lib.osi_resnet50_destroy(h)


def test_backward_ex_argument_errors(net):
    lib = N.lib()
    p, g, ws, dl, dx = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24
    bex = lib.osi_resnet50_backward_ex
    assert bex(None, p, g, ws, dl, None, dx, 1, 0, 4, None) == ERR_ARG
    assert bex(net, None, g, ws, dl, None, dx, 1, 0, 4, None) == ERR_ARG
    assert bex(net, p, g, None, dl, None, dx, 1, 0, 4, None) == ERR_ARG
    assert bex(net, p, None, ws, dl, None, dx, 1, 0, 4, None) == ERR_ARG     # parameter gradients wanted without a gradient arena
    assert bex(net, p, g, ws, dl, None, None, 0, 0, 4, None) == ERR_ARG      # neither dimage nor parameter gradients: nothing to do
    assert bex(net, p, g, ws, dl, None, dx, 2, 0, 4, None) == ERR_ARG        # param_grads is 0 or 1
    assert bex(net, p, g, ws, dl, None, dx + 2, 1, 0, 4, None) == ERR_ARG    # dimage is fp32
    assert bex(net, p, g, ws, dl, None, dx, 1, 0, 5, None) == ERR_ARG        # stage range
    assert bex(net, p, g, ws, dl, None, dx, 1, 2, 2, None) == ERR_ARG
    # well-formed (input-only, grads = NULL) but no forward has run: the executor's state check, still nothing launched
    assert bex(net, p, None, ws, dl, None, dx, 0, 0, 4, None) == ERR_STATE
    # the old entry point is the default request of the new one
    assert lib.osi_resnet50_backward(net, p, None, ws, dl, None, 0, 4, None) == ERR_ARG
    assert lib.osi_resnet50_backward(net, p, g, ws, dl, None, 0, 4, None) == ERR_STATE


def test_torch_op_registered():
    import torch
    N.ops()
    assert hasattr(torch.ops.osi, "resnet50_backward_ex")
    schema = str(torch.ops.osi.resnet50_backward_ex.default._schema)
    assert "dimage" in schema and "param_grads" in schema

"""The two-waves-per-SIMD Winograd weight gradient (csrc/conv_wino.hip, k_wino_wgrad: every 32 x 32 block of a 64 x 64 unit is shared by
two waves that own 8 of the 16 transform-domain positions each and swap accumulator halves through LDS for dW = G^T S G), and the
forward / in-block input-gradient forms beside it, through the C ABI against torch-CPU fp64 under the standing per-kernel bound
|err| <= (2e-6 + 6e-8 sqrt(K)) max|ref| + 1e-6 (tests/test_production_shapes_gpu.py), on geometries tests/test_wino_gpu.py does not
run: odd and non-square images (7 x 7, 13 x 9, 5 x 5), tile counts that are no multiple of 8 or of 64, one K step, an odd number of K
steps (the K loop is unrolled by two), B = 1 and B = 3, Cin != Cout, a stream-K remainder plan. Every comparison is over the whole
tensor; the weight gradient is in addition asserted per tap and per 32 x 32 block of every 64 x 64 unit, so that a wrong position half,
a wrong exchange slot or a wrong accumulator row cannot hide behind another block's maximum.
"""
import ctypes

import pytest
import torch

from test_production_shapes_gpu import _bound, _cpu64, _gen
from test_wino_gpu import _both_directions_cut, _dgrad, _fwd, _signed_input, _signed_wgrad_zeros  # noqa: F401  (the fixture: input-gradient pieces + fix-up stay covered)

pytestmark = pytest.mark.gpu


def _wgrad_blocks(cuda, B, H, W, Cin, Cout, act, seed, kind="positive"):
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    g = _gen(cuda, "wino-two-wave-wgrad", seed, B, H, W, Cin, Cout, act)
    d = N.ConvDesc.make(B, H, W, Cin, Cout, 3, 1, 1)
    nb = L.osi_conv_wgrad_wino_workspace(ctypes.byref(d))
    assert nb > 0
    x = torch.randn(B, H, W, Cin, device=cuda, generator=g) * 1.2 + 0.3
    dy = torch.randn(B, H, W, Cout, device=cuda, generator=g)
    a64 = _cpu64(x)
    sc = sh = None
    if act:
        sc, sh = torch.rand(Cin, device=cuda, generator=g) + 0.5, torch.randn(Cin, device=cuda, generator=g) * 0.5
        if kind == "signed":
            sc, sh = _signed_input(T, x, Cin, g, cuda)
        a64 = torch.relu(_cpu64(x) * _cpu64(sc) + _cpu64(sh))
    ws = torch.full((nb // 4,), float("nan"), device=cuda)
    outs = []
    for _ in range(2):
        dw = torch.full((Cout, 3, 3, Cin), float("nan"), device=cuda)
        N.check(L.osi_conv_wgrad_wino(ctypes.byref(d), N.ptr(dy), N.ptr(x), N.ptr(sc) if act else None, N.ptr(sh) if act else None, N.ptr(dw),
                                      N.ptr(ws), nb, T.S()), "osi_conv_wgrad_wino")
        torch.cuda.synchronize()
        outs.append(dw)
    ref = torch.nn.grad.conv2d_weight(T.nchw(a64), (Cout, Cin, 3, 3), T.nchw(_cpu64(dy)), 1, 1).permute(0, 2, 3, 1)
    err = (_cpu64(outs[0]) - ref).abs()
    bound = _bound(B * H * W, ref)
    worst = []
    for r in range(3):
        for s in range(3):
            for kb in range(Cout // 32):
                for cb in range(Cin // 32):
                    e = float(err[32 * kb:32 * kb + 32, r, s, 32 * cb:32 * cb + 32].max())
                    worst.append(e)
                    assert e <= bound, f"{(B, H, W, Cin, Cout)} tap ({r}, {s}) block ({kb}, {cb}): {e:.3e} > {bound:.3e}"
    print(f"wgrad {(B, H, W, Cin, Cout, act)}: max err {max(worst):.3e} = {max(worst) / bound:.3f} of the bound")
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]), "the same call twice: equal bits"
    if kind == "signed":
        _signed_wgrad_zeros(T, a64, ref, Cin)


def test_non_square_signed_state(cuda):
    """The non-square 13 x 9 geometry on the signed BatchNorm state (negative / zero / saturated scales, zero-variance producer
    channels): the weight gradient per tap and block at (3, 13, 9, 64, 64), the widest the Winograd weight gradient takes at that
    geometry here (it needs Cout % 64 == 0), and the in-block input gradient at (3, 13, 9, 64, 96)."""
    _wgrad_blocks(cuda, 3, 13, 9, 64, 64, True, 0, kind="signed")
    a = _dgrad(cuda, 3, 13, 9, 64, 96, 3, kind="signed")
    b = _dgrad(cuda, 3, 13, 9, 64, 96, 3, kind="signed")
    assert torch.equal(a, b), "the same call twice: equal bits"


@pytest.mark.parametrize("B,H,W,Cin,Cout,act", [
    (1, 4, 4, 64, 64, True),        # 4 tiles: ONE K step, half of it dead tiles
    (1, 7, 7, 64, 128, True),       # 16 tiles over the border: two K steps, two cout blocks
    (1, 13, 9, 128, 64, False),     # 35 tiles (no multiple of 8): five K steps, the last one ragged; plain input
    (3, 13, 9, 64, 64, True),       # 105 tiles in two splits of seven K steps
    (3, 7, 7, 192, 64, True),       # 48 tiles; three cin blocks
    (3, 5, 5, 64, 192, False),      # 27 tiles, odd image, three cout blocks
    (8, 13, 9, 128, 128, True),     # 280 tiles: five splits of seven steps, 2 x 2 units
    (5, 14, 14, 64, 64, True),      # 245 tiles, even image: four splits of 62 tiles = eight steps, the last two tiles of each dead
])
def test_weight_gradient_every_tap_and_block(cuda, B, H, W, Cin, Cout, act):
    _wgrad_blocks(cuda, B, H, W, Cin, Cout, act, 0)


@pytest.mark.parametrize("B,H,W,Cin,Cout,act", [
    (1, 7, 7, 64, 64, True),        # 16 tiles: a quarter of one unit; B = 1
    (1, 7, 7, 64, 64, False),       # the same, plain input
    (3, 7, 7, 128, 64, True),       # 48 tiles, one unit of 8 K slices on the whole chip: a stream-K remainder, every piece through the fix-up
    (3, 7, 7, 32, 128, False),      # Cin != Cout, the 32-tile x 128-channel unit where it is enabled
    (1, 5, 5, 48, 64, True),        # 9 tiles, one statistics group of 25 pixels
    (16, 6, 10, 64, 192, True),     # non-square, 240 tiles (no multiple of 64), three column units
])
def test_forward_with_statistics(cuda, B, H, W, Cin, Cout, act):
    """Forward with and without the fused input activation; _fwd checks y over the whole tensor, the BatchNorm partials and their merge,
    and that the run without statistics gives the same bits."""
    _fwd(cuda, B, H, W, Cin, Cout, act, 2)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [
    (1, 7, 7, 64, 64),              # B = 1
    (3, 13, 9, 64, 96),             # 105 tiles, non-square odd image, Cin != Cout
    (1, 13, 9, 128, 48),            # 35 tiles; the 128-channel unit where it is enabled
    (3, 7, 7, 64, 160),             # one unit of ten K slices: stream-K pieces + fix-up with the fused epilogue
])
def test_in_block_input_gradient(cuda, B, H, W, Cin, Cout):
    a = _dgrad(cuda, B, H, W, Cin, Cout, 3)
    b = _dgrad(cuda, B, H, W, Cin, Cout, 3)
    assert torch.equal(a, b), "the same call twice: equal bits"

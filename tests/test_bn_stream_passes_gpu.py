"""The element-wise BatchNorm passes of a training step (csrc/bn.hip) on every form they take for a channel count, and the one-pass
backward of a projection block's two BatchNorms.

A streaming pass walks [M][C] in tiles of 256 float4; the channel group of float4 #i is i % (C / 4). For C / 4 dividing 256 the
coefficient vectors are loaded once per lane (C = 64: 16 groups, C = 1024: 256 groups = one tile), for C = 2048 (512 groups = two tiles)
two sets are kept and picked by the parity of the TILE index under the descending walk, every other C (96: 24 groups) takes them per
element. M = 5 is shorter than one tile at C = 64, 37 and 1031 leave a ragged last tile, and 256 / 1031 give an even / odd tile count at
C = 64 (C = 2048 always has an even one: a row is two tiles). A grid of 7 workgroups makes one workgroup walk tiles of both parities.

Bounds: those of tests/test_kernels_gpu.py::test_batchnorm (_check_vs64 from there: as close to fp64 as torch-CPU fp32 is, times the
slack that test uses), everything that is a statement about wiring is exact (torch.equal)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


class _knobs:
    """tuning knobs for the duration of a block, restored afterwards"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from openset_imagenet import _native as N
        self.prev = {}
        for k, v in self.kv.items():
            p = ctypes.c_int()
            N.check(N.lib().osi_get_tuning(k.encode(), ctypes.byref(p)))
            self.prev[k] = p.value
            N.check(N.lib().osi_set_tuning(k.encode(), v))

    def __exit__(self, *exc):
        from openset_imagenet import _native as N
        for k, v in self.prev.items():
            N.check(N.lib().osi_set_tuning(k.encode(), v))


def _mask_bits(mask, n4):
    """ReLU bitmask (u64 words [(i >> 6) * 4 + component], bit i & 63) -> bool [n4][4]"""
    w = np.frombuffer(mask.cpu().numpy().tobytes(), dtype=np.uint64).reshape(-1, 4)
    i = np.arange(n4)
    return torch.from_numpy(((w[i >> 6] >> (i & 63).astype(np.uint64)[:, None]) & np.uint64(1)).astype(bool))


@pytest.mark.parametrize("kind", ["positive", "signed"])
@pytest.mark.parametrize("M", [5, 37, 256, 1031])
@pytest.mark.parametrize("C,grid", [(64, 0), (1024, 0), (2048, 0), (96, 0), (2048, 7), (64, 7)])
def test_streaming_passes_on_every_channel_geometry(cuda, C, grid, M, kind):
    """Forward block-output pass (residual + ReLU + bitmask, and the fused-shortcut form) and the backward apply (plain, bitmask-gated,
    emitting g) against torch-CPU fp64; the same call twice gives the same bits. grid = 7: the knobs bn_grid / bn_grid_bwd cap both
    passes at 7 workgroups (an odd grid: every workgroup alternates between the two coefficient sets of C = 2048)."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    from test_kernels_gpu import _check_vs64
    L = N.lib()
    g = torch.Generator().manual_seed(C * 31 + M)
    y = torch.randn(M, C, generator=g) * 2 + torch.randn(1, C, generator=g) * 5
    gamma, beta = T.bn_state(C, g, kind)
    if kind == "signed":
        y[:, T.dead_channels(C)] = 0
    resid = torch.randn(M, C, generator=g)
    dout = torch.randn(M, C, generator=g)
    y2 = torch.randn(M, C, generator=g) * 1.5 + 0.5              # the shortcut's pre-BN tensor of the fused-shortcut form
    sc2, sh2 = torch.rand(C, generator=g) - 0.3, torch.randn(C, generator=g)

    def ref(dt):   # [M][C] rows = the N*H*W axis of batch_norm
        yy = y.to(dt).t().reshape(1, C, M).clone().requires_grad_(True)
        ga, be = gamma.to(dt).clone().requires_grad_(True), beta.to(dt).clone().requires_grad_(True)
        o = F.batch_norm(yy, None, None, ga, be, True, 0.1, 1e-5)
        o.backward(dout.to(dt).t().reshape(1, C, M))
        back = lambda t: t.detach().reshape(C, M).t()
        return back(o), back(yy.grad), ga.grad, be.grad
    r32, r64 = ref(torch.float32), ref(torch.float64)

    dev = lambda t: t.to(cuda).contiguous()
    yg, ga, be, rg, dog, y2g, sc2g, sh2g = (dev(t) for t in (y, gamma, beta, resid, dout, y2, sc2, sh2))
    mean, invstd, scale, shift = (torch.empty(C, device=cuda) for _ in range(4))
    wsb = max(L.osi_bn_workspace(M, C), L.osi_bn_backward_workspace(M, C))
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    N.check(L.osi_bn_train_stats(N.ptr(yg), M, C, N.ptr(ga), N.ptr(be), 1e-5, 0.1, None, None, N.ptr(mean), N.ptr(invstd), N.ptr(scale),
                                 N.ptr(shift), N.ptr(ws), wsb, T.S()))
    n4 = M * C // 4
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    knobs = _knobs(bn_grid=grid, bn_grid_bwd=grid) if grid else _knobs()
    with knobs:
        # ---- forward block-output pass
        outs, masks = [], []
        for _ in range(2):
            out, mask = nan(M, C), torch.zeros(L.osi_bn_relu_mask_bytes(M, C), dtype=torch.uint8, device=cuda)
            N.check(L.osi_bn_apply_relu_mask(N.ptr(yg), N.ptr(rg), N.ptr(scale), N.ptr(shift), N.ptr(out), N.ptr(mask), M, C, T.S()))
            outs.append(out); masks.append(mask)
        out, mask = outs[0], masks[0]
        assert torch.equal(outs[0], outs[1]) and torch.equal(masks[0], masks[1]), "the same call twice: the same bits"
        # the reference takes the ReLU decisions the kernel took (an element within rounding of zero may fall either way)
        bits = _mask_bits(mask, n4).reshape(M, C)
        pre32, pre64 = r32[0] + resid, r64[0] + resid.double()
        _check_vs64(out, pre32 * bits, pre64 * bits, "block output")
        assert torch.equal(bits, out.cpu() > 0), "bitmask = (output > 0)"
        # (and those may differ from the fp64 decisions only where the pre-activation is within the output's own error of zero: the bound
        # above is at least 2e-6 of the tensor's scale, 1e-5 leaves room for the reference side's share)
        off = bits != (pre64 > 0)
        assert float(pre64[off].abs().max() if off.any() else 0.0) <= 1e-5 * float(pre64.abs().max()), "a ReLU decision away from zero differs"
        # fused-shortcut form = the shortcut's BatchNorm applied first, then the residual form: bit for bit (include/osi.h)
        short, o_a, o_b = nan(M, C), nan(M, C), nan(M, C)
        m_a, m_b = torch.zeros_like(mask), torch.zeros_like(mask)
        N.check(L.osi_bn_apply(N.ptr(y2g), None, N.ptr(sc2g), N.ptr(sh2g), N.ptr(short), M, C, 0, T.S()))
        N.check(L.osi_bn_apply_relu_mask(N.ptr(yg), N.ptr(short), N.ptr(scale), N.ptr(shift), N.ptr(o_a), N.ptr(m_a), M, C, T.S()))
        N.check(L.osi_bn_apply_relu_mask2(N.ptr(yg), N.ptr(scale), N.ptr(shift), N.ptr(y2g), N.ptr(sc2g), N.ptr(sh2g), N.ptr(o_b), N.ptr(m_b),
                                          M, C, T.S()))
        assert torch.equal(o_a, o_b) and torch.equal(m_a, m_b), "fused-shortcut block output"
        _check_vs64(short, y2 * sc2 + sh2, y2.double() * sc2.double() + sh2.double(), "plain apply")

        # ---- backward apply, ungated, emitting g
        res = []
        for _ in range(2):
            dy, gm, dg, db = nan(M, C), nan(M, C), nan(C), nan(C)
            N.check(L.osi_bn_backward(N.ptr(dog), None, N.ptr(yg), N.ptr(mean), N.ptr(invstd), N.ptr(ga), N.ptr(dy), N.ptr(gm), N.ptr(dg),
                                      N.ptr(db), M, C, N.ptr(ws), wsb, T.S()))
            res.append((dy, gm, dg, db))
        dy, gm, dg, db = res[0]
        assert all(torch.equal(a, b) for a, b in zip(*res)), "the same call twice: the same bits"
        assert torch.equal(gm, dog)
        _check_vs64(dy, r32[1], r64[1], "bn dy", slack=8.0, floor=5e-6)
        _check_vs64(dg, r32[2], r64[2], "bn dgamma", slack=8.0, floor=5e-6)
        _check_vs64(db, r32[3], r64[3], "bn dbeta", slack=8.0, floor=5e-6)
        # ---- gated by the forward's bitmask: g = dout * bit exactly, and everything else is the ungated pass on that g, bit for bit
        dy2, gm2, dg2, db2 = nan(M, C), nan(M, C), nan(C), nan(C)
        N.check(L.osi_bn_backward_relu_mask(N.ptr(dog), N.ptr(mask), N.ptr(yg), N.ptr(mean), N.ptr(invstd), N.ptr(ga), N.ptr(dy2), N.ptr(gm2),
                                            N.ptr(dg2), N.ptr(db2), M, C, N.ptr(ws), wsb, T.S()))
        assert torch.equal(gm2.cpu(), torch.where(bits, dout, torch.zeros(())))
        dy3, dg3, db3 = nan(M, C), nan(C), nan(C)
        N.check(L.osi_bn_backward(N.ptr(gm2), None, N.ptr(yg), N.ptr(mean), N.ptr(invstd), N.ptr(ga), N.ptr(dy3), None, N.ptr(dg3), N.ptr(db3),
                                  M, C, N.ptr(ws), wsb, T.S()))
        assert torch.equal(dy2, dy3) and torch.equal(dg2, dg3) and torch.equal(db2, db3), "gated pass = ungated pass on the gated gradient"
        # in place (dy aliases the gradient)
        N.check(L.osi_bn_backward(N.ptr(gm2), None, N.ptr(yg), N.ptr(mean), N.ptr(invstd), N.ptr(ga), N.ptr(gm2), None, N.ptr(dg3), N.ptr(db3),
                                  M, C, N.ptr(ws), wsb, T.S()))
        assert torch.equal(gm2, dy3), "in-place backward"
    torch.cuda.synchronize()
    if kind == "signed":
        assert torch.isfinite(dy).all() and torch.isfinite(dg).all() and torch.isfinite(db).all() and torch.isfinite(out).all()
        assert float(dy[:, gamma == 0].abs().max()) == 0 and float(dy2[:, gamma == 0].abs().max()) == 0, "gamma = 0: dy exactly 0"


# P = 1, 3, 70: one launch finishes the sums (P <= bn_wide_p = 2048). The two-level form (group sums, then one wave per channel) is
# taken beyond that limit: 2049 is the smallest P that takes it at the default limit, and 70 takes it with the limit lowered to 64.
# grid = 7 / 8: the apply pass capped at that many workgroups, so that every workgroup walks several tiles (odd: both parities at C = 2048).
@pytest.mark.parametrize("P,wide_p,grid", [(1, None, 0), (3, None, 0), (70, None, 0), (70, 64, 0), (2049, None, 0), (3, None, 7), (3, None, 8)])
@pytest.mark.parametrize("C,M", [(256, 4 * 7 * 7), (2048, 2 * 7 * 7)])
def test_two_consumer_backward_equals_two_single_passes(cuda, C, M, P, wide_p, grid):
    """osi_bn_backward_fused2 (one pass over g for bn3 and the shortcut's BatchNorm, one finalising launch for both) against two
    osi_bn_backward_fused calls on the same inputs: both dy tensors, dgamma and dbeta of both consumers, bit for bit."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    gen = torch.Generator().manual_seed(C + 7 * P + M)
    dev = lambda t: t.to(cuda).contiguous()
    g = dev(torch.randn(M, C, generator=gen))
    psum_g = dev(torch.randn(P, C, generator=gen))
    cons = []
    for k in range(2):
        gamma, _ = T.bn_state(C, gen, "signed")            # negative and zero scales included
        cons.append(dict(y=dev(torch.randn(M, C, generator=gen) * 2 + 1), mean=dev(torch.randn(C, generator=gen)),
                         invstd=dev(torch.rand(C, generator=gen) + 0.5), gamma=dev(gamma), psum_gx=dev(torch.randn(P, C, generator=gen))))
    wsb = max(L.osi_bn_backward_workspace(M, C), L.osi_bn_backward_fused2_workspace(C), (2 * 32 * C + 2 * C) * 4)
    ws = torch.full((wsb // 4,), float("nan"), device=cuda)
    nan = lambda *s: torch.full(s, float("nan"), device=cuda)
    kv = {}
    if wide_p is not None:
        kv["bn_wide_p"] = wide_p
    if grid:
        kv["bn_grid_bwd"] = grid
    with _knobs(**kv):
        single = []
        for c in cons:
            dy, dg, db = nan(M, C), nan(C), nan(C)
            N.check(L.osi_bn_backward_fused(N.ptr(g), N.ptr(c["y"]), N.ptr(c["mean"]), N.ptr(c["invstd"]), N.ptr(c["gamma"]), N.ptr(psum_g),
                                            N.ptr(c["psum_gx"]), P, N.ptr(dy), N.ptr(dg), N.ptr(db), M, C, N.ptr(ws), wsb, T.S()))
            single.append((dy, dg, db))
        ws.fill_(float("nan"))
        pair = [(nan(M, C), nan(C), nan(C)) for _ in cons]
        table = (N.BnFusedConsumer * 2)(*[N.BnFusedConsumer(N.ptr(c["y"]), N.ptr(c["mean"]), N.ptr(c["invstd"]), N.ptr(c["gamma"]),
                                                            N.ptr(c["psum_gx"]), N.ptr(o[0]), N.ptr(o[1]), N.ptr(o[2]))
                                          for c, o in zip(cons, pair)])
        N.check(L.osi_bn_backward_fused2(N.ptr(g), table, N.ptr(psum_g), P, M, C, N.ptr(ws), wsb, T.S()), "osi_bn_backward_fused2")
        torch.cuda.synchronize()
        for k in range(2):
            for a, b, what in zip(single[k], pair[k], ("dy", "dgamma", "dbeta")):
                assert torch.isfinite(b).all(), f"{what} of consumer {k}: unwritten or non-finite elements"
                assert torch.equal(a, b), f"{what} of consumer {k} differs from the single-consumer pass"
        assert torch.equal(pair[0][2], pair[1][2]), "dbeta = sum g is the same for both consumers"
        # consumer 0 may write over g
        g2 = g.clone()
        table[0].dy = N.ptr(g2)
        N.check(L.osi_bn_backward_fused2(N.ptr(g2), table, N.ptr(psum_g), P, M, C, N.ptr(ws), wsb, T.S()), "osi_bn_backward_fused2 in place")
        torch.cuda.synchronize()
        assert torch.equal(g2, single[0][0]) and torch.equal(pair[1][0], single[1][0]), "in-place form"
    # refused before any launch: the second dy aliasing the gradient or the first dy
    table[1].dy = N.ptr(g2)
    assert L.osi_bn_backward_fused2(N.ptr(g2), table, N.ptr(psum_g), P, M, C, N.ptr(ws), wsb, T.S()) == -1


PROJECTION_TENSORS = [f"resnet_base.layer{s}.0.{t}" for s in (1, 2, 3, 4)
                      for t in ("conv3.weight", "downsample.0.weight", "bn3.weight", "bn3.bias", "downsample.1.weight", "downsample.1.bias")]


class _NoComm:
    """stand-in for the data-parallel gradient sync at world size 1: the model takes its stage-by-stage backward"""

    def bucket_ready(self, flat, lo, hi, handoff=None):
        pass

    def finish(self):
        pass


def test_projection_block_gradients_one_call_vs_staged_backward(cuda):
    """B = 2 at 64 x 64 through the executor: the gradients of every projection block's conv3, shortcut convolution and both
    BatchNorms (the tensors behind the one-pass backward) are the same bits from a one-call and from a staged backward, and every
    gradient of both is within the whole-network gate (tests/test_gate_pinned_gpu.py: 5e-4 relative L2 per tensor against the fp64
    oracle under the HIP path's own ReLU / arg-max decisions)."""
    from openset_imagenet import ResNet50, EntropicOpensetLoss
    from oracle import resnet50_oracle as R, losses_oracle as Lo
    from osi_testlib import hip_gates
    from test_gate_pinned_gpu import GRAD_TOL, _rel
    B, HW, C = 2, 64, 10
    gen = torch.Generator().manual_seed(97)
    sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), generator=gen)
    model = ResNet50(C, C, False)
    model.load_state_dict(sd)
    model = model.to(cuda).train()
    x = torch.rand(B, 3, HW, HW, generator=gen)
    y = torch.tensor([3, -1])
    loss = EntropicOpensetLoss(C, 1.0)

    def step():
        model.zero_grad()
        logits, _ = model(x.to(cuda))
        loss(logits, y.to(cuda)).backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    one = step()
    gates = hip_gates(model)
    model._grad_sync = _NoComm()
    try:
        staged = step()
    finally:
        model._grad_sync = None
    for k in PROJECTION_TENSORS:
        assert k in one, k
        assert torch.equal(one[k], staged[k]), f"{k}: one-call and staged backward differ"
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    g64 = R.forward_backward(sd64, x.double(), y, lambda lg, t, f: Lo.entropic_openset_loss(lg, t, 1.0), gates=gates)[3]
    for tag, got in (("one call", one), ("staged", staged)):
        errs = {k: _rel(got[k], g64[k]) for k in R.param_keys(sd)}
        worst = max(errs, key=errs.get)
        print(f"{tag}: gradient rel-L2 vs fp64 under the HIP gates: median {np.median(list(errs.values())):.2e} max {errs[worst]:.2e} ({worst})")
        assert len(errs) == 162
        for k, e in errs.items():
            assert e <= GRAD_TOL, f"{tag}: grad {k}: rel-L2 {e:.2e} > {GRAD_TOL:.0e} under pinned gates"

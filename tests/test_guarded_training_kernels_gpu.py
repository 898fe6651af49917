"""The training kernels behind the C ABI under the harness the detector kernels already have (tests/gpu_harness.py): every output
between canary bands and pre-filled with NaN, every input between 0xFF bands (a NaN in fp32: a halo load that reaches an accumulator
shows in the output), every workspace of exactly the bytes its own query names, between bands, and its contents never assumed.

Each case makes the same calls (three_fills): (a) workspace full of 0xFF, (b) a fresh one full of 0x00, (c) the workspace of (a)
again after a call of the same entry point on OTHER values left its data in it. After every call: status OK, all bands whole, no input
written, no NaN in an output. Across the calls: the same bits. Against the reference: the fp64 arithmetic and the bound of the
kernel's existing parity test (imported, not restated): _check_vs64 with the floor 2e-6 + 6e-8 sqrt(K) of tests/test_kernels_gpu.py,
_bound of tests/test_production_shapes_gpu.py, and where a kernel's test states another bound, that one, named at the assertion.

Shapes are the smallest that have the edge in question (ragged last row tile, halo on every side, a parity class that is ragged,
M below one tile, a partial last mask word); the cases assert that the edge is there. None uses the benchmarked batch."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpu_harness as H
from test_kernels_gpu import _check_vs64
from test_production_shapes_gpu import _bound, _xhat_sums

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, U8, I32 = torch.float32, torch.uint8, torch.int32
OSI_ERR_ARG = -1


def _libs():
    import osi_testlib as T
    from openset_imagenet import _native as N
    return N.lib(), N, T


def tile_band(C):
    """Trailing band of one 128-row tile of a [rows][C] fp32 tensor: a store from the far side of a phantom tile lands in it."""
    return (128 * C * 4 + 255) // 256 * 256


def fl(K):
    """The floor of tests/test_kernels_gpu.py for an exact-f32 fma chain of length K."""
    return 2e-6 + 6e-8 * K ** 0.5


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def gen(*seed):
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


class _Ptrs(dict):
    """Device pointers by attribute: `i.x`; None stays None (a NULL argument). `i.t["x"]`: the tensor itself, for the call wrappers of
    osi_testlib."""
    __getattr__ = dict.__getitem__

    def __init__(self, bufs):
        super().__init__({k: None if v is None else v.t.data_ptr() for k, v in bufs.items()})
        self.__dict__["t"] = {k: None if v is None else v.t for k, v in bufs.items()}


def status_of(call):
    """Status of a call made through a wrapper of osi_testlib (they raise where the library refuses): 0, or the code in the error."""
    import re
    try:
        call()
        return 0
    except RuntimeError as e:
        m = re.search(r"\(code (-?\d+)\)", str(e))
        if m is None:
            raise
        return int(m.group(1))


def _make_out(spec, dev):
    """spec: (shape, dtype[, trailing band]) = an output, NaN-filled when it is a float; a CPU tensor[, trailing band] = a buffer the
    call reads AND writes (an accumulate target, an optimizer state, a documented pre-fill), uploaded with its bits."""
    if isinstance(spec, torch.Tensor):
        spec = (spec,)
    if isinstance(spec[0], torch.Tensor):
        o = H.Out(tuple(spec[0].shape), spec[0].dtype, dev, band=(H.GUARD, spec[1] if len(spec) > 1 else H.GUARD))
        o.t.copy_(spec[0])
        return o
    shape, dtype = spec[0], spec[1]
    return H.Out(shape, dtype, dev, band=(H.GUARD, spec[2] if len(spec) > 2 else H.GUARD), fill=NAN if dtype.is_floating_point else None)


def _once(dev, launch, inputs, outs, ws, refusable=False):
    """One guarded call. launch(i, o, w) -> status, or (status, extras): extras["ws_out"] = {workspace name: leading floats of it that
    are an output (partials)}, extras["info"] = anything the caller wants back. Returns (outputs as numpy by name, info), or None when
    the call was refused with OSI_ERR_ARG and `refusable`: then nothing at all may have been written."""
    ins = {k: None if v is None else H.In(v, dev) for k, v in inputs.items()}
    o = {k: _make_out(s, dev) for k, s in outs.items()}
    before = {k: v.t.clone() for k, v in o.items()}
    ret = launch(_Ptrs(ins), _Ptrs(o), ws)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:            # a store that missed every band: the device is in an error state, nothing more is started on it
        pytest.exit(f"GPU fault in a guarded call: {e}", returncode=3)
    rc, extras = ret if isinstance(ret, tuple) else (ret, {})
    for k, v in ins.items():
        assert v is None or v.unchanged(), f"input {k}: written, or a band around it"
    for k, v in o.items():
        assert v.check(), f"output {k}: a store outside it"
    for k, v in ws.items():
        assert v.check(), f"workspace {k} ({v.nbytes} bytes): a store outside it"
    if refusable and rc == OSI_ERR_ARG:
        for k, v in o.items():
            assert H.same_bytes(v.t.cpu().numpy().view(np.uint8), before[k].cpu().numpy().view(np.uint8)), f"refused, yet output {k} was written"
        return None
    assert rc == 0, f"status {rc}"
    res = {k: v.np().copy() for k, v in o.items()}
    for k, n in extras.get("ws_out", {}).items():
        assert 4 * n <= ws[k].nbytes
        res["ws:" + k] = ws[k].t[:4 * n].cpu().numpy().view(np.float32).copy()
    for k, a in res.items():
        assert a.dtype.kind != "f" or not np.isnan(a).any(), f"{k}: NaN in the output (an element not written, or a halo value used)"
    return res, extras.get("info", {})


def _same(a, b):
    return H.same_bits_nan(a, b) if a.dtype == np.float32 else H.same_bytes(a, b)


def three_fills(dev, launch, inputs, other, outs, ws_bytes=None, band=H.GUARD, refusable=False, ws_in=None):
    """The three calls of the module docstring. ws_bytes: {name: bytes} (launch gets {name: H.Ws}: .ptr, .nbytes). ws_in: {workspace
    name: input name}: the header makes the LEADING part of that workspace an input (the partials osi_bn_finalize_stats merges); the
    named input's bits are put there before every call, the rest keeps the fill / the stale data. Returns (outputs of call (a), info of
    call (a), the workspaces of (a) and (c) as they are after (c)), or None when call (a) was refused (`refusable`)."""
    mk = lambda fill: {k: H.Ws(n, dev, fill=fill, band=band) for k, n in (ws_bytes or {}).items()}

    def call(inp, ws, refusable=False):
        for k, src in (ws_in or {}).items():
            bits = inp[src].contiguous().reshape(-1).view(U8)
            ws[k].t[:bits.numel()].copy_(bits)
        return _once(dev, launch, {k: v for k, v in inp.items() if k not in (ws_in or {}).values()}, outs, ws, refusable)
    wa = mk(0xFF)
    first = call(inputs, wa, refusable)
    if first is None:
        return None
    a, info = first
    b, info_b = call(inputs, mk(0x00))
    call(other, wa)
    c, info_c = call(inputs, wa)
    assert info == info_b == info_c
    for k in a:
        assert _same(a[k], b[k]), f"{k}: a workspace of 0x00 gives other bits than one of 0xFF"
        assert _same(a[k], c[k]), f"{k}: the data an earlier call left in the workspace changes the result"
    return a, info, wa


# ---- implicit GEMM (csrc/conv_igemm.hip) ---------------------------------------------------------------------------------------------
# (B, Cin, Cout, k, stride, H)
CONV = [(3, 64, 64, 1, 1, 9),        # M = 243: ragged for 64-row and 128-row tiles
        (3, 64, 128, 3, 1, 7),       # halo on every side, M = 147
        (3, 128, 128, 3, 2, 9),      # odd size, stride 2: a ragged parity class of the input gradient
        (5, 64, 128, 1, 2, 7),       # the sparse input gradient
        (2, 256, 64, 1, 1, 5)]       # M = 50: less than one tile
conv_ids = lambda s: "x".join(map(str, s))


class _Conv:
    """Inputs (NHWC / KRSC, fp32 on the CPU) of one convolution shape from a seeded generator, and its fp32 / fp64 torch references."""

    def __init__(self, shape, seed=0):
        _, N, T = _libs()
        B, Cin, Cout, k, stride, Hh = shape
        self.shape, self.pad = shape, 1 if k == 3 else 0
        g = gen("conv", shape, seed)
        self.d = N.ConvDesc.make(B, Hh, Hh, Cin, Cout, k, stride, self.pad)
        self.M, self.Mi = B * self.d.Ho * self.d.Wo, B * Hh * Hh
        self.x = torch.randn(B, Hh, Hh, Cin, generator=g) + 0.2
        self.w = torch.randn(Cout, k, k, Cin, generator=g) / (Cin * k * k) ** 0.5
        self.dy = torch.randn(B, self.d.Ho, self.d.Wo, Cout, generator=g)
        self.base = torch.randn(B, Hh, Hh, Cin, generator=g)                      # accumulate target / addend
        # scale and shift of a fused input activation as tests/test_tail_split_gpu.py draws them
        self.sc, self.sh = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.5
        self.res = torch.randn(B, Hh, Hh, Cin, generator=g)
        self.osc, self.osh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.5     # epilogue coefficients
        self.ores = torch.randn(B, self.d.Ho, self.d.Wo, Cout, generator=g)
        self.yshape, self.xshape = (B, self.d.Ho, self.d.Wo, Cout), (B, Hh, Hh, Cin)

    def fwd(self, dt, act=0):
        """conv2d of x (act 0), relu(x sc + sh) (1) or relu(x sc + sh + res) (2), NHWC, in dtype dt"""
        _, _, T = _libs()
        a = self.x.to(dt)
        if act:
            a = a * self.sc.to(dt) + self.sh.to(dt)
            a = torch.relu(a + self.res.to(dt) if act == 2 else a)
        s = self.shape
        return F.conv2d(T.nchw(a), T.oihw(self.w.to(dt)), None, s[4], self.pad).permute(0, 2, 3, 1).contiguous()

    def dgrad(self, dt):
        _, _, T = _libs()
        s = self.shape
        return torch.nn.grad.conv2d_input((s[0], s[1], s[5], s[5]), T.oihw(self.w.to(dt)), T.nchw(self.dy.to(dt)), s[4], self.pad).permute(0, 2, 3, 1).contiguous()

    def wgrad(self, dt, act=0):
        _, _, T = _libs()
        s = self.shape
        a = self.x.to(dt)
        if act:
            a = torch.relu(a * self.sc.to(dt) + self.sh.to(dt))
        return torch.nn.grad.conv2d_weight(T.nchw(a), (s[2], s[1], s[3], s[3]), T.nchw(self.dy.to(dt)), s[4], self.pad).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv(shape, seed=0):
    return _Conv(shape, seed)


def _ragged(M):
    return M % 64 != 0 and M % 128 != 0


@pytest.mark.parametrize("shape", CONV, ids=conv_ids)
def test_conv_fwd_every_tile(cuda, shape):
    L, N, T = _libs()
    c, c2 = conv(shape), conv(shape, 1)
    assert _ragged(c.M), "the last row tile is meant to be ragged"
    K = shape[1] * shape[3] ** 2
    y32, y64 = c.fwd(F32), c.fwd(torch.float64)
    taken = []
    for tile in range(9):
        run = lambda i, o, w: status_of(lambda: T.conv_fwd(i.t["x"], i.t["w"], shape[3], shape[4], c.pad, tile, y=o.t["y"]))
        r = three_fills(cuda, run, dict(x=c.x, w=c.w), dict(x=c2.x, w=c2.w), dict(y=(c.yshape, F32, tile_band(shape[2]))), refusable=True)
        if r is not None:
            taken.append(tile)
            _check_vs64(tt(r[0]["y"]), y32, y64, f"conv fwd tile {tile}", floor=fl(K))
    assert {0, 2, 4} <= set(taken) and (shape[2] % 128 != 0 or {1, 3} <= set(taken)), taken


def _check_row_partials(ps, P, rows, y, C, scale):
    """Per-row-tile (mean, M2) of THIS output y [M][C], the bounds of tests/test_tail_split_gpu.py."""
    M = y.shape[0]
    assert (P - 1) * rows < M <= P * rows
    ps = tt(ps).double()
    pm, pq = ps[:P * C].view(P, C), ps[P * C:2 * P * C].view(P, C)
    for t in range(P):
        r = y[t * rows:min(M, (t + 1) * rows)]
        assert torch.allclose(pm[t], r.mean(0), atol=2e-6 * scale), t
        assert torch.allclose(pq[t], ((r - r.mean(0)) ** 2).sum(0), rtol=1e-4, atol=1e-5), t


def _fwd_stats_launch(L, T, c, which, tile, stats=True):
    """osi_conv_fwd_bnstats (which 0), osi_conv_fwd_act (1), osi_conv_fwd_act2 (2) with the partials in workspace "ps"."""
    def run(i, o, w):
        P, rows = ctypes.c_int(-1), ctypes.c_int(-1)
        ps, nb = (w["ps"].ptr, w["ps"].nbytes) if stats else (None, 0)
        tail = (ps, nb, ctypes.byref(P) if stats else None, ctypes.byref(rows) if stats else None, T.S())
        if which == 0:
            rc = L.osi_conv_fwd_bnstats(ctypes.byref(c.d), i.x, i.w, o.y, tile, *tail)
        elif which == 1:
            rc = L.osi_conv_fwd_act(ctypes.byref(c.d), i.x, i.sc, i.sh, i.w, o.y, tile, *tail)
        else:
            rc = L.osi_conv_fwd_act2(ctypes.byref(c.d), i.x, i.sc, i.sh, i.res, i.w, o.y, tile, *tail)
        if rc != 0 or not stats:
            return rc
        return rc, dict(ws_out=dict(ps=2 * P.value * c.shape[2]), info=dict(P=P.value, rows=rows.value))
    return run


def _fwd_inputs(c, which):
    d = dict(x=c.x, w=c.w)
    if which:
        d.update(sc=c.sc, sh=c.sh)
    if which == 2:
        d.update(res=c.res)
    return d


@pytest.mark.parametrize("which", [0, 1, 2], ids=["bnstats", "act", "act2"])
@pytest.mark.parametrize("shape", CONV, ids=conv_ids)
def test_conv_fwd_with_statistics_and_fused_input(cuda, shape, which):
    L, N, T = _libs()
    c, c2 = conv(shape), conv(shape, 1)
    Cout, K = shape[2], shape[1] * shape[3] ** 2
    y32, y64 = c.fwd(F32, which), c.fwd(torch.float64, which)
    nb = L.osi_conv_fwd_bnstats_workspace(ctypes.byref(c.d))
    assert nb >= 2 * ((c.M + 63) // 64) * Cout * 4
    taken = []
    for tile in range(9):
        for stats in (True, False) if which else (True,):
            r = three_fills(cuda, _fwd_stats_launch(L, T, c, which, tile, stats), _fwd_inputs(c, which), _fwd_inputs(c2, which),
                            dict(y=(c.yshape, F32, tile_band(Cout))), dict(ps=nb) if stats else None, band=tile_band(Cout), refusable=True)
            if r is None:
                continue
            taken.append((tile, stats))
            _check_vs64(tt(r[0]["y"]), y32, y64, f"tile {tile} stats {stats}", floor=fl(K))
            if stats:
                _check_row_partials(r[0]["ws:ps"], r[1]["P"], r[1]["rows"], tt(r[0]["y"]).double().view(c.M, Cout), Cout, float(y64.abs().max()))
    if which == 2 and not (shape[3] == 1 and shape[4] == 1):
        assert not taken, "osi_conv_fwd_act2 is the 1x1 stride-1 form: every other shape is refused"
    else:
        assert (0, True) in taken and (which == 0 or (0, False) in taken) and (5, True) in taken, taken


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shape", CONV, ids=conv_ids)
def test_conv_fwd_epilogue(cuda, shape, residual):
    L, N, T = _libs()
    c, c2 = conv(shape), conv(shape, 1)
    Cout, K = shape[2], shape[1] * shape[3] ** 2
    nb = L.osi_conv_fwd_epilogue_workspace(ctypes.byref(c.d))

    def ref(dt):
        v = c.fwd(dt) * c.osc.to(dt) + c.osh.to(dt)
        return torch.relu(v + c.ores.to(dt) if residual else v)

    def run(i, o, w):
        e = N.ConvEpilogue(i.osc, i.osh, i.ores, 1)
        return L.osi_conv_fwd_epilogue(ctypes.byref(c.d), i.x, i.w, o.out, ctypes.byref(e), w["ws"].ptr, w["ws"].nbytes, T.S())
    ins = lambda v: dict(x=v.x, w=v.w, osc=v.osc, osh=v.osh, ores=v.ores if residual else None)
    for ws in sorted({nb, 0}):           # the slab of the plan in force, and none (single pass, as the header allows)
        r = three_fills(cuda, run, ins(c), ins(c2), dict(out=(c.yshape, F32, tile_band(Cout))), dict(ws=ws), band=tile_band(64))
        _check_vs64(tt(r[0]["out"]), ref(F32), ref(torch.float64), f"epilogue ws {ws}", floor=fl(K))


def _reached(c):
    """bool [H][H]: the input pixels some filter tap reaches."""
    B, Cin, Cout, k, s, Hh = c.shape
    ones = torch.nn.grad.conv2d_input((1, 1, Hh, Hh), torch.ones(1, 1, k, k, dtype=torch.float64), torch.ones(1, 1, c.d.Ho, c.d.Wo, dtype=torch.float64), s, c.pad)
    return ones[0, 0] > 0


@pytest.mark.parametrize("accumulate", [0, 1, 2])
@pytest.mark.parametrize("shape", CONV, ids=conv_ids)
def test_conv_dgrad_every_tile(cuda, shape, accumulate):
    L, N, T = _libs()
    c, c2 = conv(shape), conv(shape, 1)
    B, Cin, Cout, k, s, Hh = shape
    assert _ragged(B * ((Hh + s - 1) // s) ** 2) or _ragged(c.Mi)
    K = Cout * k * k
    hit = _reached(c)
    dx32, dx64 = c.dgrad(F32), c.dgrad(torch.float64)
    if accumulate == 1:
        dx32, dx64 = dx32 + c.base, dx64 + c.base.double()
    if accumulate == 2:                  # pixels no tap reaches keep the bits the buffer held
        keep = (~hit).view(1, Hh, Hh, 1)
        dx32, dx64 = torch.where(keep, c.base, dx32), torch.where(keep, c.base.double(), dx64)
        assert shape != CONV[3] or int(hit.sum()) == ((Hh + 1) // 2) ** 2, "a stride-2 1x1 convolution reaches the even-even pixels"
    spec = (c.base, tile_band(Cin)) if accumulate else (c.xshape, F32, tile_band(Cin))
    taken = []
    for tile in range(9):
        run = lambda i, o, w: status_of(lambda: T.conv_dgrad(i.t["dy"], i.t["w"], Hh, Hh, k, s, c.pad, accumulate_into=o.t["dx"], tile=tile, accumulate=accumulate))
        r = three_fills(cuda, run, dict(dy=c.dy, w=c.w), dict(dy=c2.dy, w=c2.w), dict(dx=spec), refusable=True)
        if r is None:
            continue
        taken.append(tile)
        got = tt(r[0]["dx"])
        _check_vs64(got, dx32, dx64, f"dgrad accumulate {accumulate} tile {tile}", floor=fl(K))
        if accumulate == 2:
            assert torch.equal(got[:, ~hit], c.base[:, ~hit]), "sparse form: an untouched pixel changed"
        elif accumulate == 0 and bool((~hit).any()):
            assert float(got[:, ~hit].abs().max()) == 0, "a pixel no tap reaches has a zero gradient"
    assert {0, 2, 4} <= set(taken) and (Cin % 128 != 0 or {1, 3} <= set(taken)), taken


# the five shapes have M <= 245: one K split, no slab. Two more whose weight gradient really goes through the workspace (M = 588: three
# splits of whole 32-row blocks, the last one ragged), per-tap and all-taps form
WGRAD_SPLIT = [(3, 64, 64, 1, 1, 14), (3, 64, 64, 3, 1, 14)]


@pytest.mark.parametrize("act", [0, 1], ids=["wgrad", "wgrad_act"])
@pytest.mark.parametrize("shape", CONV + WGRAD_SPLIT, ids=conv_ids)
def test_conv_wgrad(cuda, shape, act):
    L, N, T = _libs()
    c, c2 = conv(shape), conv(shape, 1)
    B, Cin, Cout, k, s, Hh = shape
    nb = L.osi_conv_wgrad_workspace(ctypes.byref(c.d))
    if shape in WGRAD_SPLIT:
        assert nb >= 2 * Cout * k * k * Cin * 4 and c.M % 32 != 0, "this case is meant to split K, with a ragged last split"

    def run(i, o, w):
        if act:
            return L.osi_conv_wgrad_act(ctypes.byref(c.d), i.dy, i.x, i.sc, i.sh, o.dw, w["ws"].ptr, w["ws"].nbytes, T.S())
        return status_of(lambda: T.conv_wgrad(i.t["dy"], i.t["x"], k, s, c.pad, dw=o.t["dw"], ws=w["ws"].t))
    ins = lambda v: dict(dy=v.dy, x=v.x, **(dict(sc=v.sc, sh=v.sh) if act else {}))
    r = three_fills(cuda, run, ins(c), ins(c2), dict(dw=((Cout, k, k, Cin), F32, tile_band(Cin))), dict(ws=nb), band=tile_band(64))
    _check_vs64(tt(r[0]["dw"]), c.wgrad(F32, act), c.wgrad(torch.float64, act), "wgrad", floor=fl(c.M))


def pack_mask(gate, nbytes):
    """The ReLU bitmask of osi_bn_apply_relu_mask for gate (bool, [M][C] flattened): element 4 i + c is bit i % 64 of 64-bit word
    4 (i / 64) + c (the layout tests/test_kernels_gpu.py unpacks)."""
    g = np.asarray(gate, dtype=bool).reshape(-1, 4)
    words = np.zeros((nbytes // 32, 4), dtype=np.uint64)
    i = np.arange(g.shape[0])
    for ch in range(4):
        np.bitwise_or.at(words[:, ch], i >> 6, g[:, ch].astype(np.uint64) << (i & 63).astype(np.uint64))
    return torch.from_numpy(words.view(np.uint8).reshape(-1).copy())


def unpack_mask(mask_u8, n):
    words = np.asarray(mask_u8).view(np.uint64).reshape(-1, 4)
    i = np.arange(n // 4)
    return np.stack([(words[i >> 6, ch] >> (i & 63).astype(np.uint64)) & 1 for ch in range(4)], axis=1).reshape(-1).astype(bool)


class _Gate:
    """What the fused input-gradient epilogues read about the producer of the convolution's input: the pre-BN tensor(s) y0 (y1), their
    statistics, and the ReLU gate as a bitmask or as scale0 / shift0 to recompute it from (pre-activations 1e-3 away from zero, so
    fp32 and fp64 agree on every decision, as tests/test_production_shapes_gpu.py draws them)."""

    def __init__(self, M, C, seed, mask_bytes):
        g = gen("gate", M, C, seed)
        self.sc, self.sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
        pre = torch.randn(M, C, generator=g)
        pre = torch.where(pre >= 0, pre.clamp_min(1e-3), pre.clamp_max(-1e-3))
        self.y0 = ((pre.double() - self.sh.double()) / self.sc.double()).float()
        self.gate = pre > 0
        self.mask = pack_mask(self.gate.numpy(), mask_bytes)
        self.y1 = torch.randn(M, C, generator=g) * 2 + 0.5
        st = lambda y: (y.double().mean(0).float(), (1 / torch.sqrt(y.double().var(0, unbiased=False) + 1e-5)).float())
        (self.mean0, self.inv0), (self.mean1, self.inv1) = st(self.y0), st(self.y1)


def _check_partial_sums(ps, P, C, g64, consumers):
    """Column sums over the row tiles of sum g and sum g * xhat_i against fp64: the bounds of tests/test_production_shapes_gpu.py."""
    p = tt(ps).double().view(-1, P, C)
    assert float(((p[0].sum(0) - g64.sum(0)).abs() / (g64.abs().sum(0) + 1e-3)).max()) <= 1e-5, "sum g"
    for j, (y, mean, inv) in enumerate(consumers):
        _, sgx, l1 = _xhat_sums(g64, y, mean, inv)
        assert float(((p[1 + j].sum(0) - sgx).abs() / (l1 + 1e-3)).max()) <= 2e-5, f"sum g * xhat{j}"


@pytest.mark.parametrize("form", ["mask", "mask2", "gate", "frozen"])
@pytest.mark.parametrize("shape", CONV, ids=conv_ids)
def test_conv_dgrad_fused(cuda, shape, form):
    """osi_conv_dgrad_fused with the gate from the bitmask (one and two BatchNorm consumers, with the addend) and recomputed from the
    pre-BN tensor, and osi_conv_dgrad_fused_frozen; the partial sums are the leading part of the workspace the query sizes."""
    L, N, T = _libs()
    c, c2 = conv(shape), conv(shape, 1)
    B, Cin, Cout, k, s, Hh = shape
    M = c.Mi
    mb = L.osi_bn_relu_mask_bytes(M, Cin)
    q, q2 = _Gate(M, Cin, 0, mb), _Gate(M, Cin, 1, mb)
    two, planes = form == "mask2", 2 if form == "frozen" else 3
    pb = L.osi_conv_dgrad_fused_workspace(ctypes.byref(c.d))
    assert pb > 0

    def ins(v, qq):
        d = dict(dy=v.dy, w=v.w, y0=qq.y0, mean0=qq.mean0, inv0=qq.inv0)
        if form in ("mask", "mask2"):
            d.update(mask=qq.mask, addend=v.base)
            if two:
                d.update(y1=qq.y1, mean1=qq.mean1, inv1=qq.inv1)
        else:
            d.update(sc=qq.sc, sh=qq.sh)
        return d

    def launch(partials):
        def run(i, o, w):
            f = T.Fusion(i.get("mask"), i.y0, i.mean0, i.inv0, i.get("y1"), i.get("mean1"), i.get("inv1"), w["parts"].ptr if partials else None,
                         w["parts"].nbytes if partials else 0, i.get("sc"), i.get("sh"), None, 0, 0, 1)
            P = ctypes.c_int(-1)
            if form == "frozen":
                rc = L.osi_conv_dgrad_fused_frozen(ctypes.byref(c.d), i.dy, i.w, o.dx, ctypes.byref(f), 0, ctypes.byref(P), T.S())
            else:
                rc = L.osi_conv_dgrad_fused(ctypes.byref(c.d), i.dy, i.w, o.dx, i.get("addend"), ctypes.byref(f), 0, ctypes.byref(P), T.S())
            if rc != 0 or not partials:
                return rc
            return rc, dict(ws_out=dict(parts=(2 + two) * P.value * Cin), info=dict(P=P.value))
        return run

    g64 = c.dgrad(torch.float64)
    if form in ("mask", "mask2"):
        g64 = g64 + c.base.double()
    g64 = (g64 * q.gate.view(c.xshape)).view(M, Cin)
    ref = g64 * q.sc.double() if form == "frozen" else g64
    r = three_fills(cuda, launch(True), ins(c, q), ins(c2, q2), dict(dx=(c.xshape, F32, tile_band(Cin))), dict(parts=pb), band=tile_band(Cin),
                    refusable=form in ("gate", "frozen"))
    if r is None:
        assert s != 1, "the in-block forms take every stride-1 shape"
        return
    got = tt(r[0]["dx"]).double().view(M, Cin)
    assert float((got - ref).abs().max()) <= _bound(Cout * k * k, ref)
    assert bool((got[~q.gate] == 0).all()), "exact zeros behind a closed gate"
    P = r[1]["P"]
    assert P >= (M + 127) // 128 and planes * P * Cin * 4 <= pb
    _check_partial_sums(r[0]["ws:parts"], P, Cin, g64, [(q.y0, q.mean0, q.inv0)] + ([(q.y1, q.mean1, q.inv1)] if two else []))
    if form == "frozen":                 # the input-only form: no partials, nothing but dx written, the same bits
        r0 = three_fills(cuda, launch(False), ins(c, q), ins(c2, q2), dict(dx=(c.xshape, F32, tile_band(Cin))))
        got = tt(r0[0]["dx"]).double().view(M, Cin)
        assert float((got - ref).abs().max()) <= _bound(Cout * k * k, ref) and bool((got[~q.gate] == 0).all())


def test_conv_dgrad_fused_pool_mode(cuda):
    """Pool mode at the shape of tests/test_stem_tail_gpu.py (2 x 16 x 16 x 64 before the pool): dx = input gradient + addend, the
    partial sums = bn1's reductions through the arg-max bytes (fp64 as tests/test_production_shapes_gpu.py evaluates them)."""
    L, N, T = _libs()
    B, Hs, C, Cout = 2, 16, 64, 64
    Hp = (Hs + 2 - 3) // 2 + 1
    c, c2 = conv((B, C, Cout, 1, 1, Hp)), conv((B, C, Cout, 1, 1, Hp), 1)
    M = B * Hp * Hp

    def stem(seed):
        g = gen("pool", seed)
        y = torch.randn(B, Hs, Hs, C, generator=g) * 1.5 + 0.2
        bsc, bsh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
        yd, sd, hd = (t.to(cuda) for t in (y, bsc, bsh))
        pooled, idx = torch.empty(B, Hp, Hp, C, device=cuda), torch.zeros(M * C, dtype=U8, device=cuda)
        N.check(L.osi_bn_relu_maxpool_fwd(N.ptr(yd), N.ptr(sd), N.ptr(hd), N.ptr(pooled), N.ptr(idx), B, Hs, Hs, C, T.S()))
        v = y.double().view(-1, C)
        return y, idx.cpu(), v.mean(0).float(), (1 / torch.sqrt(v.var(0, unbiased=False) + 1e-5)).float()
    (y, idx, mean, inv), (y2, idx2, mean2, inv2) = stem(0), stem(1)
    pb = L.osi_conv_dgrad_fused_workspace(ctypes.byref(c.d))

    def run(i, o, w):
        f = T.Fusion(None, i.y, i.mean, i.inv, None, None, None, w["parts"].ptr, w["parts"].nbytes, None, None, i.idx, Hs, Hs, 1)
        P = ctypes.c_int(-1)
        rc = L.osi_conv_dgrad_fused(ctypes.byref(c.d), i.dy, i.w, o.dx, o.dx, ctypes.byref(f), 0, ctypes.byref(P), T.S())
        return rc if rc else (rc, dict(ws_out=dict(parts=2 * P.value * C), info=dict(P=P.value)))
    r = three_fills(cuda, run, dict(dy=c.dy, w=c.w, y=y, mean=mean, inv=inv, idx=idx), dict(dy=c2.dy, w=c2.w, y=y2, mean=mean2, inv=inv2, idx=idx2),
                    dict(dx=(c.base, tile_band(C))), dict(parts=pb), band=tile_band(C))      # dx holds the addend, completed in place
    ref = c.dgrad(torch.float64) + c.base.double()
    assert float((tt(r[0]["dx"]).double() - ref).abs().max()) <= _bound(Cout, ref)
    by = idx.view(B, Hp, Hp, C).long()
    tap = by & 0x7F
    assert bool((by >> 7).any()) and not bool((by >> 7).all())
    ho, wo = torch.arange(Hp).view(1, Hp, 1, 1), torch.arange(Hp).view(1, 1, Hp, 1)
    flat = ((2 * ho - 1 + tap // 3) * Hs + (2 * wo - 1 + tap % 3)).clamp_(0, Hs * Hs - 1)
    yarg = y.double().view(B, Hs * Hs, C).gather(1, flat.view(B, Hp * Hp, C)).view(B, Hp, Hp, C)
    gv = ref * (by >> 7).double()
    xh = (yarg - mean.double()) * inv.double()
    P = r[1]["P"]
    p = tt(r[0]["ws:parts"]).double().view(2, P, C)
    assert float(((p[0].sum(0) - gv.view(M, C).sum(0)).abs() / (gv.view(M, C).abs().sum(0) + 1e-3)).max()) <= 1e-5
    assert float(((p[1].sum(0) - (gv * xh).view(M, C).sum(0)).abs() / ((gv * xh).abs().view(M, C).sum(0) + 1e-3)).max()) <= 2e-5


# ---- the K-split tail: plans that really split (tests/test_tail_split_gpu.py) -----------------------------------------------------
def _macs(row, dgrad):
    Cin, Cout, k = row[0], row[1], row[2]
    B, Hh, stride = (row[4], row[3], 1) if dgrad else (row[5], row[4], row[3])
    return B * ((Hh + stride - 1) // stride) ** 2 * Cin * Cout * k * k


def _two_smallest(rows, dgrad):
    return sorted(rows, key=lambda r: _macs(r, dgrad))[:2]


def _tail_rows(dgrad):
    import test_tail_split_gpu as TS
    return _two_smallest(TS.DCASES if dgrad else TS.CASES, dgrad)


@pytest.mark.parametrize("row", _tail_rows(False), ids=conv_ids)
def test_forward_tail_split(cuda, row):
    """The two rows of CASES with the fewest multiply-adds, under their tail_cus / tail_mint / tail_smax: the slab behind the statistics
    is part of the queried workspace, the split run differs from the un-split one in bits but not beyond the bound, and a caller who
    offers only the un-split size gets the un-split bits."""
    L, N, T = _libs()
    Cin, Cout, k, stride, Hh, B, cus, fused = row
    shape = (B, Cin, Cout, k, stride, Hh)
    c, c2 = conv(shape), conv(shape, 1)
    y32, y64 = c.fwd(F32, fused), c.fwd(torch.float64, fused)
    outs = dict(y=(c.yshape, F32, tile_band(Cout)))
    with T.pinned_knobs(tail_cus=cus, tail_mint=2, tail_smax=32):
        nb = L.osi_conv_fwd_bnstats_workspace(ctypes.byref(c.d))
        with T.pinned_knobs(tail_split=0):
            nb0 = L.osi_conv_fwd_bnstats_workspace(ctypes.byref(c.d))
            r0 = three_fills(cuda, _fwd_stats_launch(L, T, c, fused, 0), _fwd_inputs(c, fused), _fwd_inputs(c2, fused), outs, dict(ps=nb0), band=tile_band(Cout))
        assert nb > nb0, "this case is meant to have a split remainder (the workspace grows by the slab)"
        r1 = three_fills(cuda, _fwd_stats_launch(L, T, c, fused, 0), _fwd_inputs(c, fused), _fwd_inputs(c2, fused), outs, dict(ps=nb), band=tile_band(Cout))
        r3 = three_fills(cuda, _fwd_stats_launch(L, T, c, fused, 0), _fwd_inputs(c, fused), _fwd_inputs(c2, fused), outs, dict(ps=nb0), band=tile_band(Cout))
    for r in (r0, r1):
        _check_vs64(tt(r[0]["y"]), y32, y64, "tail", floor=fl(Cin * k * k))
        assert float((tt(r[0]["y"]).double() - y64).abs().max()) <= (2e-6 + 6e-8 * (Cin * k * k) ** 0.5) * float(y64.abs().max()) + 1e-6
        _check_row_partials(r[0]["ws:ps"], r[1]["P"], r[1]["rows"], tt(r[0]["y"]).double().view(c.M, Cout), Cout, float(y64.abs().max()))
    assert r0[1] == r1[1] == dict(P=(c.M + 63) // 64, rows=64)
    assert not H.same_bits_nan(r1[0]["y"], r0[0]["y"]), "the split really changed the summation order of some tile"
    assert H.same_bits_nan(r3[0]["y"], r0[0]["y"]), "only the un-split workspace offered: the un-split launch"
    if ((c.M + 63) // 64) * (Cout // 64) >= 2 * cus:
        assert H.same_bits_nan(r1[0]["y"].reshape(c.M, Cout)[:64], r0[0]["y"].reshape(c.M, Cout)[:64]), "tiles of the full rounds are untouched"


@pytest.mark.parametrize("row", _tail_rows(True), ids=conv_ids)
def test_input_gradient_tail_split(cuda, row):
    L, N, T = _libs()
    Cin, Cout, k, Hh, B, cus, two, bits, add = row
    shape = (B, Cin, Cout, k, 1, Hh)
    c, c2 = conv(shape), conv(shape, 1)
    M = c.Mi
    mb = L.osi_bn_relu_mask_bytes(M, Cin)
    q, q2 = _Gate(M, Cin, 0, mb), _Gate(M, Cin, 1, mb)

    def ins(v, qq):
        d = dict(dy=v.dy, w=v.w, y0=qq.y0, mean0=qq.mean0, inv0=qq.inv0, addend=v.base if add else None)
        d.update(dict(mask=qq.mask) if bits else dict(sc=qq.sc, sh=qq.sh))
        if two:
            d.update(y1=qq.y1, mean1=qq.mean1, inv1=qq.inv1)
        return d

    def run(i, o, w):
        f = T.Fusion(i.get("mask"), i.y0, i.mean0, i.inv0, i.get("y1"), i.get("mean1"), i.get("inv1"), w["parts"].ptr, w["parts"].nbytes,
                     i.get("sc"), i.get("sh"), None, 0, 0, 1)
        P = ctypes.c_int(-1)
        rc = L.osi_conv_dgrad_fused(ctypes.byref(c.d), i.dy, i.w, o.dx, i.addend, ctypes.byref(f), 0, ctypes.byref(P), T.S())
        return rc if rc else (rc, dict(ws_out=dict(parts=(2 + two) * P.value * Cin), info=dict(P=P.value)))
    outs = dict(dx=(c.xshape, F32, tile_band(Cin)))
    with T.pinned_knobs(tail_cus=cus, tail_mint=2, tail_smax=32):
        pb = L.osi_conv_dgrad_fused_workspace(ctypes.byref(c.d))
        with T.pinned_knobs(tail_split=0):
            pb0 = L.osi_conv_dgrad_fused_workspace(ctypes.byref(c.d))
            r0 = three_fills(cuda, run, ins(c, q), ins(c2, q2), outs, dict(parts=pb0), band=tile_band(Cin))
        assert pb > pb0, "this case is meant to have a split remainder"
        r1 = three_fills(cuda, run, ins(c, q), ins(c2, q2), outs, dict(parts=pb), band=tile_band(Cin))
    g64 = c.dgrad(torch.float64) + (c.base.double() if add else 0)
    g64 = (g64 * q.gate.view(c.xshape)).view(M, Cin)
    tol = (2e-6 + 6e-8 * (Cout * k * k) ** 0.5) * float(g64.abs().max()) + 1e-6
    for r in (r0, r1):
        got = tt(r[0]["dx"]).double().view(M, Cin)
        assert float((got - g64).abs().max()) <= tol and bool((got[~q.gate] == 0).all())
        assert r[1]["P"] == (M + 63) // 64
        _check_partial_sums(r[0]["ws:parts"], r[1]["P"], Cin, g64, [(q.y0, q.mean0, q.inv0)] + ([(q.y1, q.mean1, q.inv1)] if two else []))
    assert not H.same_bits_nan(r1[0]["dx"], r0[0]["dx"]), "the split really changed the summation order of some tile"


# ---- BatchNorm (csrc/bn.hip) ---------------------------------------------------------------------------------------------------------
BN_SHAPES = [(180, 12), (147, 256)]             # 5 x 6 x 6 and 3 x 7 x 7: M is no multiple of 64 (partial last mask word, partial row tile)
MERGE_KNOBS = dict(bn_grid=1, bn_grid_bwd=1, bn_single_p=1, bn_wide_p=0)      # the merges of partials take their two-level form


class _Bn:
    """One BatchNorm layer's tensors ([M][C] fp32 on the CPU) and its references in a given dtype."""

    def __init__(self, M, C, seed=0):
        g = gen("bn", M, C, seed)
        self.M, self.C = M, C
        self.y = torch.randn(M, C, generator=g) * 2 + torch.randn(1, C, generator=g) * 5
        self.gamma, self.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        self.rm, self.rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        self.res, self.dout = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
        self.y_b = torch.randn(M, C, generator=g) * 1.5 + 0.5                  # the projection shortcut's pre-BN tensor
        self.gamma_b, self.beta_b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        # what the kernels downstream of the statistics are given: fp32 roundings of the fp64 statistics
        self.mean, self.inv, self.scale, self.shift = (t.float() for t in self.stats(torch.float64)[:4])
        self.mean_b, self.inv_b, self.scale_b, self.shift_b = (t.float() for t in self.stats(torch.float64, "b")[:4])
        self.P = (M + 63) // 64                                                   # 64-row tiles, as a convolution's epilogue emits partials

    def stats(self, dt, which="a"):
        y, ga, be = (self.y, self.gamma, self.beta) if which == "a" else (self.y_b, self.gamma_b, self.beta_b)
        y, ga, be = y.to(dt), ga.to(dt), be.to(dt)
        mean, var = y.mean(0), y.var(0, unbiased=False)
        inv = 1 / torch.sqrt(var + 1e-5)
        return mean, inv, ga * inv, be - mean * ga * inv, 0.9 * self.rm.to(dt) + 0.1 * mean, 0.9 * self.rv.to(dt) + 0.1 * var * self.M / (self.M - 1)

    def tile_stats(self):
        """[P][C] means then [P][C] M2 of the 64-row tiles, fp32, as one tensor: the pstats of osi_bn_finalize_stats"""
        t = [self.y.double()[i * 64:(i + 1) * 64] for i in range(self.P)]
        return torch.cat([torch.stack([v.mean(0) for v in t]), torch.stack([((v - v.mean(0)) ** 2).sum(0) for v in t])]).float().contiguous()

    def apply(self, dt, relu, res):
        """res: None, "id" (identity shortcut) or "bn" (the shortcut's own BatchNorm on the fly)"""
        v = self.y.to(dt) * self.scale.to(dt) + self.shift.to(dt)
        if res == "id":
            v = v + self.res.to(dt)
        if res == "bn":
            v = v + (self.y_b.to(dt) * self.scale_b.to(dt) + self.shift_b.to(dt))
        return torch.relu(v) if relu else v

    def backward(self, dt, gate, which="a"):
        """(g, dy, dgamma, dbeta) of the gated gradient g = dout . gate through the BatchNorm `which`, statistics as given to the kernels"""
        y, mean, inv, ga = ((self.y, self.mean, self.inv, self.gamma) if which == "a" else (self.y_b, self.mean_b, self.inv_b, self.gamma_b))
        y, mean, inv, ga = y.to(dt), mean.to(dt), inv.to(dt), ga.to(dt)
        g = self.dout.to(dt) * gate.to(dt)
        xh = (y - mean) * inv
        db, dg = g.sum(0), (g * xh).sum(0)
        return g, ga * inv * (g - db / self.M - xh * dg / self.M), dg, db

    def tile_sums(self, gate, which="a"):
        """[P][C] per-tile sums of g and of g * xhat (fp32): what a dgrad epilogue hands to the fused backward"""
        g, _, _, _ = self.backward(torch.float64, gate, which)
        y, mean, inv = (self.y, self.mean, self.inv) if which == "a" else (self.y_b, self.mean_b, self.inv_b)
        gx = g * ((y.double() - mean.double()) * inv.double())
        cut = lambda v: torch.stack([v[i * 64:(i + 1) * 64].sum(0) for i in range(self.P)]).float().contiguous()
        return cut(g), cut(gx)


@functools.lru_cache(maxsize=None)
def bn(M, C, seed=0):
    return _Bn(M, C, seed)


def _knobs(T, merge):
    import contextlib
    return T.pinned_knobs(**MERGE_KNOBS) if merge else contextlib.nullcontext()


def _touched(ws, fill=0xFF):
    """Bytes of a workspace that no longer hold the fill of call (a)."""
    return int((ws.t != fill).sum())


bn_params = pytest.mark.parametrize("merge", [False, True], ids=["default", "two-level"])
bn_shapes = pytest.mark.parametrize("M,C", BN_SHAPES)
BWD = dict(slack=8.0, floor=5e-6)         # the backward bounds of tests/test_kernels_gpu.py::_batchnorm_case


@bn_shapes
@bn_params
def test_bn_train_stats(cuda, M, C, merge):
    L, N, T = _libs()
    b, b2 = bn(M, C), bn(M, C, 1)
    nb = L.osi_bn_workspace(M, C)
    assert nb > 0 and M % 64 != 0

    def run(i, o, w):
        return L.osi_bn_train_stats(i.y, M, C, i.gamma, i.beta, 1e-5, 0.1, o.rm, o.rv, o.mean, o.inv, o.scale, o.shift, w["ws"].ptr, w["ws"].nbytes, T.S())
    ins = lambda v: dict(y=v.y, gamma=v.gamma, beta=v.beta)
    vec = ((C,), F32)
    with _knobs(T, merge):
        r = three_fills(cuda, run, ins(b), ins(b2), dict(rm=b.rm, rv=b.rv, mean=vec, inv=vec, scale=vec, shift=vec), dict(ws=nb))
    assert _touched(r[2]["ws"]) > 0, "the partials go through the workspace"
    for name, r32, r64 in zip(("mean", "inv", "scale", "shift", "rm", "rv"), b.stats(F32), b.stats(torch.float64)):
        _check_vs64(tt(r[0][name]), r32, r64, name)


@bn_shapes
@bn_params
def test_bn_finalize_stats(cuda, M, C, merge):
    """pstats = [P][C] means, [P][C] M2, then the scratch of the two-level merge: (2 P + 64) C floats in all (include/osi.h)."""
    L, N, T = _libs()
    b, b2 = bn(M, C), bn(M, C, 1)
    P = b.P
    assert P > 1 and M % 64 != 0
    nb = (2 * P + 64) * C * 4

    def run(i, o, w):
        return L.osi_bn_finalize_stats(w["ps"].ptr, w["ps"].nbytes, P, 64, M, C, i.gamma, i.beta, 1e-5, 0.1, o.rm, o.rv, o.mean, o.inv, o.scale, o.shift, T.S())
    ins = lambda v: dict(ps=v.tile_stats(), gamma=v.gamma, beta=v.beta)
    vec = ((C,), F32)
    with _knobs(T, merge):
        r = three_fills(cuda, run, ins(b), ins(b2), dict(rm=b.rm, rv=b.rv, mean=vec, inv=vec, scale=vec, shift=vec), dict(ps=nb), ws_in=dict(ps="ps"))
        assert L.osi_bn_finalize_stats(r[2]["ps"].ptr, nb - 4, P, 64, M, C, *[r[2]["ps"].ptr] * 2, 1e-5, 0.1, None, None, *[r[2]["ps"].ptr] * 4, T.S()) == OSI_ERR_ARG
    assert H.same_bytes(r[2]["ps"].t[:2 * P * C * 4].cpu().numpy(), b.tile_stats().view(-1).view(U8).numpy()), "the partials are only read"
    scratch = r[2]["ps"].t[2 * P * C * 4:]
    assert bool((scratch != 0xFF).any()) == merge, "the two-level merge, and only it, goes through the scratch behind the partials"
    for name, r32, r64 in zip(("mean", "inv", "scale", "shift", "rm", "rv"), b.stats(F32), b.stats(torch.float64)):
        _check_vs64(tt(r[0][name]), r32, r64, name)


@bn_shapes
@bn_params
@pytest.mark.parametrize("form", ["plain", "relu", "relu+res", "mask", "mask+res", "mask2"])
def test_bn_apply_forms(cuda, M, C, merge, form):
    """osi_bn_apply, osi_bn_apply_relu_mask, osi_bn_apply_relu_mask2: the mask is an output of exactly osi_bn_relu_mask_bytes(M, C)."""
    L, N, T = _libs()
    b, b2 = bn(M, C), bn(M, C, 1)
    mb = L.osi_bn_relu_mask_bytes(M, C)
    # 180 x 12: 540 units of 4 floats = 8 mask words and 28 bits of a ninth. 147 x 256 fills its 147 words (64 units per row) exactly
    assert M % 64 != 0 and ((M * C // 4) % 64 != 0 or C == 256), "the last mask word of the small shape is meant to be partial"
    res = "bn" if form == "mask2" else "id" if form.endswith("+res") else None
    relu = form != "plain"

    def run(i, o, w):
        if form == "mask2":
            return L.osi_bn_apply_relu_mask2(i.y, i.scale, i.shift, i.y_b, i.scale_b, i.shift_b, o.out, o.mask, M, C, T.S())
        if form.startswith("mask"):
            return L.osi_bn_apply_relu_mask(i.y, i.res, i.scale, i.shift, o.out, o.mask, M, C, T.S())
        return L.osi_bn_apply(i.y, i.res, i.scale, i.shift, o.out, M, C, int(relu), T.S())
    ins = lambda v: dict(y=v.y, scale=v.scale, shift=v.shift, res=v.res if res == "id" else None, **(dict(y_b=v.y_b, scale_b=v.scale_b, shift_b=v.shift_b) if res == "bn" else {}))
    outs = dict(out=((M, C), F32, tile_band(C)))
    if form.startswith("mask"):
        outs["mask"] = ((mb,), U8)
    with _knobs(T, merge):
        r = three_fills(cuda, run, ins(b), ins(b2), outs)
    _check_vs64(tt(r[0]["out"]), b.apply(F32, relu, res), b.apply(torch.float64, relu, res), form)
    if form.startswith("mask"):
        assert np.array_equal(unpack_mask(r[0]["mask"], M * C), r[0]["out"].reshape(-1) > 0), "the bitmask is (out > 0), bit for bit"


@bn_shapes
@bn_params
@pytest.mark.parametrize("form", ["none", "act", "mask"])
def test_bn_backward_forms(cuda, M, C, merge, form):
    """osi_bn_backward (no gate / gate from the activation) and osi_bn_backward_relu_mask."""
    L, N, T = _libs()
    b, b2 = bn(M, C), bn(M, C, 1)
    nb = L.osi_bn_backward_workspace(M, C)
    mb = L.osi_bn_relu_mask_bytes(M, C)
    act = lambda v: v.apply(F32, True, "id")
    gate = lambda v: act(v) > 0 if form != "none" else torch.ones(M, C, dtype=torch.bool)

    def run(i, o, w):
        if form == "mask":
            return L.osi_bn_backward_relu_mask(i.dout, i.mask, i.y, i.mean, i.inv, i.gamma, o.dy, o.gm, o.dg, o.db, M, C, w["ws"].ptr, w["ws"].nbytes, T.S())
        return L.osi_bn_backward(i.dout, i.get("act"), i.y, i.mean, i.inv, i.gamma, o.dy, o.gm, o.dg, o.db, M, C, w["ws"].ptr, w["ws"].nbytes, T.S())
    ins = lambda v: dict(dout=v.dout, y=v.y, mean=v.mean, inv=v.inv, gamma=v.gamma,
                         **(dict(act=act(v)) if form == "act" else dict(mask=pack_mask(gate(v).numpy(), mb)) if form == "mask" else {}))
    big, vec = ((M, C), F32, tile_band(C)), ((C,), F32)
    with _knobs(T, merge):
        r = three_fills(cuda, run, ins(b), ins(b2), dict(dy=big, gm=big, dg=vec, db=vec), dict(ws=nb))
    assert _touched(r[2]["ws"]) > 0
    r32, r64 = b.backward(F32, gate(b)), b.backward(torch.float64, gate(b))
    assert torch.equal(tt(r[0]["gm"]), r32[0]), "gmasked is the gated gradient itself"
    for j, name in ((1, "dy"), (2, "dg"), (3, "db")):
        _check_vs64(tt(r[0][name]), r32[j], r64[j], name, **BWD)


@bn_shapes
@bn_params
@pytest.mark.parametrize("form", ["fused", "fused2", "reduce"])
def test_bn_backward_from_partial_sums(cuda, M, C, merge, form):
    """osi_bn_backward_fused, osi_bn_backward_fused2 and osi_bn_backward_reduce on [P][C] row-tile sums (P = 3: a partial last tile).
    Bound: 2e-5 of the tensor's scale, as tests/test_kernels_gpu.py::_dgrad_fused_case holds the fused route to."""
    L, N, T = _libs()
    b, b2 = bn(M, C), bn(M, C, 1)
    P = b.P
    nb = L.osi_bn_backward_fused2_workspace(C) if form == "fused2" else L.osi_bn_backward_workspace(M, C)
    gate = lambda v: v.apply(F32, True, "id") > 0
    g32 = lambda v: v.backward(F32, gate(v))[0]

    def run(i, o, w):
        ws, n = w["ws"].ptr, w["ws"].nbytes
        if form == "reduce":
            return L.osi_bn_backward_reduce(i.sg, i.sgx, P, o.dg, o.db, M, C, ws, n, T.S())
        if form == "fused":
            return L.osi_bn_backward_fused(i.g, i.y, i.mean, i.inv, i.gamma, i.sg, i.sgx, P, o.dy, o.dg, o.db, M, C, ws, n, T.S())
        cs = (N.BnFusedConsumer * 2)(N.BnFusedConsumer(i.y, i.mean, i.inv, i.gamma, i.sgx, o.dy, o.dg, o.db),
                                     N.BnFusedConsumer(i.y_b, i.mean_b, i.inv_b, i.gamma_b, i.sgx_b, o.dy_b, o.dg_b, o.db_b))
        return L.osi_bn_backward_fused2(i.g, cs, i.sg, P, M, C, ws, n, T.S())

    def ins(v):
        sg, sgx = v.tile_sums(gate(v))
        d = dict(sg=sg, sgx=sgx)
        if form != "reduce":
            d.update(g=g32(v), y=v.y, mean=v.mean, inv=v.inv, gamma=v.gamma)
        if form == "fused2":
            d.update(y_b=v.y_b, mean_b=v.mean_b, inv_b=v.inv_b, gamma_b=v.gamma_b, sgx_b=v.tile_sums(gate(v), "b")[1])
        return d
    big, vec = ((M, C), F32, tile_band(C)), ((C,), F32)
    outs = dict(dg=vec, db=vec)
    if form != "reduce":
        outs["dy"] = big
    if form == "fused2":
        outs.update(dy_b=big, dg_b=vec, db_b=vec)
    with _knobs(T, merge):
        r = three_fills(cuda, run, ins(b), ins(b2), outs, dict(ws=nb))
    assert _touched(r[2]["ws"]) > 0, "the merged sums and the apply coefficients go through the workspace"
    # the layout of one consumer: [C][S] group sums of g and of g * xhat (S = 1 at P = 3), then the two coefficient vectors. The single
    # launch writes the coefficients only; the group sums are the two-level form's
    assert bool((r[2]["ws"].t[:2 * C * 4] != 0xFF).any()) == merge, "the two-level merge, and only it, goes through the group sums"
    for which, sfx in (("a", ""), ("b", "_b"))[:2 if form == "fused2" else 1]:
        r64 = b.backward(torch.float64, gate(b), which)
        for j, name in ((1, "dy"), (2, "dg"), (3, "db")):
            if name + sfx in r[0]:
                err = float((tt(r[0][name + sfx]).double() - r64[j]).abs().max())
                assert err <= 2e-5 * (float(r64[j].abs().max()) + 1e-30), (name + sfx, err)


@bn_shapes
@bn_params
@pytest.mark.parametrize("n,mask,sums", [(1, True, True), (2, True, True), (2, False, False), (1, False, True)])
def test_bn_backward_frozen(cuda, M, C, merge, n, mask, sums):
    """osi_bn_backward_frozen: one or two consumers, gate from the bitmask or none, with and without the parameter gradients.
    Bounds: those of tests/test_frozen_bn_gpu.py."""
    from test_frozen_bn_gpu import _bound as frozen_bound
    L, N, T = _libs()
    b, b2 = bn(M, C), bn(M, C, 1)
    nb = L.osi_bn_backward_workspace(M, C)
    mb = L.osi_bn_relu_mask_bytes(M, C)
    gate = lambda v: (v.apply(F32, True, "id") > 0) if mask else torch.ones(M, C, dtype=torch.bool)

    def run(i, o, w):
        cs = (N.BnFrozenConsumer * 2)(N.BnFrozenConsumer(i.y, i.mean, i.inv, i.scale, o.dy, o.get("dg"), o.get("db")),
                                      N.BnFrozenConsumer(i.y_b, i.mean_b, i.inv_b, i.scale_b, o.get("dy_b"), o.get("dg_b"), o.get("db_b")))
        return L.osi_bn_backward_frozen(i.dout, i.get("mask"), cs, n, o.gm, M, C, w["ws"].ptr, w["ws"].nbytes, T.S())
    ins = lambda v: dict(dout=v.dout, y=v.y, mean=v.mean, inv=v.inv, scale=v.scale, y_b=v.y_b, mean_b=v.mean_b, inv_b=v.inv_b, scale_b=v.scale_b,
                         **(dict(mask=pack_mask(gate(v).numpy(), mb)) if mask else {}))
    big, vec = ((M, C), F32, tile_band(C)), ((C,), F32)
    outs = dict(dy=big, gm=big)
    if n == 2:
        outs["dy_b"] = big
    if sums:
        outs.update(dg=vec, db=vec, **(dict(dg_b=vec, db_b=vec) if n == 2 else {}))
    with _knobs(T, merge):
        r = three_fills(cuda, run, ins(b), ins(b2), outs, dict(ws=nb))
    assert (_touched(r[2]["ws"]) > 0) == sums, "no reduction is launched without parameter gradients"
    g64 = b.dout.double() * gate(b)
    assert torch.equal(tt(r[0]["gm"]).double(), g64), "gmasked is the gated gradient itself"
    for which, sfx in (("a", ""), ("b", "_b"))[:n]:
        scale = (b.scale if which == "a" else b.scale_b).double()
        ref = g64 * scale
        got = tt(r[0]["dy" + sfx]).double()
        assert float((got - ref).abs().max()) <= frozen_bound(1, ref) and bool((got[~gate(b)] == 0).all())
        if sums:
            _, _, dg, db = b.backward(torch.float64, gate(b), which)
            for name, want in (("dg", dg), ("db", db)):
                assert float((tt(r[0][name + sfx]).double() - want).abs().max()) <= frozen_bound(M, want), name + sfx


# ---- Winograd forms (csrc/conv_wino.hip), wino_streamk = 1: both directions cut their ragged round --------------------------------
# (B, H, W, Cin, Cout)
WINO = [(6, 7, 7, 64, 128),          # tiles hang over the border; 96 tiles: the second unit is half empty
        (3, 14, 14, 64, 64),         # 147 tiles: ragged last statistics group and unit; input gradient (the forward refuses it)
        (8, 12, 20, 48, 64)]         # non-square, Cin % 16 only: forward only


class _Wino:
    def __init__(self, shape, seed=0):
        _, N, T = _libs()
        B, Hh, W, Cin, Cout = shape
        g = gen("wino", shape, seed)
        self.d = N.ConvDesc.make(B, Hh, W, Cin, Cout, 3, 1, 1)
        self.M = B * Hh * W
        self.Pn = (B * ((Hh + 1) // 2) * ((W + 1) // 2) + 15) // 16
        self.x = torch.randn(B, Hh, W, Cin, generator=g) * 1.2 + 0.3
        self.w = torch.randn(Cout, 3, 3, Cin, generator=g) / math.sqrt(Cin * 9)
        self.sc, self.sh = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.5
        self.dy = torch.randn(B, Hh, W, Cout, generator=g)
        self.wd = torch.randn(Cout, 3, 3, Cin, generator=g) / math.sqrt(Cout * 9)      # the input gradient's weights, at its scale
        self.q = _Gate(self.M, Cin, ("wino", seed), (self.M * Cin // 4 + 63) // 64 * 32)

    def fwd64(self, act):
        _, _, T = _libs()
        a = self.x.double()
        if act:
            a = torch.relu(a * self.sc.double() + self.sh.double())
        return F.conv2d(T.nchw(a), T.oihw(self.w.double()), None, 1, 1).permute(0, 2, 3, 1).contiguous()

    def dgrad64(self):
        _, _, T = _libs()
        B, Hh, W, Cin, Cout = self.d.B, self.d.H, self.d.W, self.d.Cin, self.d.Cout
        acc = torch.nn.grad.conv2d_input((B, Cin, Hh, W), T.oihw(self.wd.double()), T.nchw(self.dy.double()), 1, 1).permute(0, 2, 3, 1)
        return (acc * self.q.gate.view(B, Hh, W, Cin)).reshape(self.M, Cin)

    def wgrad64(self, act):
        _, _, T = _libs()
        a = self.x.double()
        if act:
            a = torch.relu(a * self.sc.double() + self.sh.double())
        return torch.nn.grad.conv2d_weight(T.nchw(a), (self.d.Cout, self.d.Cin, 3, 3), T.nchw(self.dy.double()), 1, 1).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def wino(shape, seed=0):
    return _Wino(shape, seed)


def _check_group_partials(ps, P, rows, C, ref):
    """(mean, M2) per 16-tile group merged in fp64 as a set against the fp64 columns: tests/test_production_shapes_gpu.py's
    _check_partials_and_finalize, its first half (every group holds `rows` pixels)."""
    M = ref.shape[0]
    assert P * rows == M
    p = tt(ps).double()
    pm, pq = p[:P * C].view(P, C), p[P * C:2 * P * C].view(P, C)
    rmean = ref.mean(0)
    rM2 = ((ref - rmean) ** 2).sum(0)
    mean = pm.mean(0)
    M2 = pq.sum(0) + (rows * (pm - mean) ** 2).sum(0)
    assert float((mean - rmean).abs().max()) <= 2e-6 * float(ref.abs().max()) + 1e-6
    assert float(((M2 - rM2).abs() / rM2).max()) <= 1e-4


def _slab_touched(ws, u_bytes):
    """Bytes of the stream-K slab that no longer hold the fill of call (a): the slab is its own workspace in the `_pre` forms and lies
    behind the transformed weights (osi_conv_wino_weights_bytes(d) bytes) in the workspace of the raw forms."""
    return _touched(ws["slab"]) if "slab" in ws else int((ws["ws"].t[u_bytes:] != 0xFF).sum())


def _wino_fwd_case(cuda, shape, act, stats, pre):
    L, N, T = _libs()
    B, Hh, W, Cin, Cout = shape
    v, v2 = wino(shape), wino(shape, 1)
    d = v.d
    ub, sb, wb = L.osi_conv_wino_weights_bytes(ctypes.byref(d)), L.osi_conv_wino_slab_bytes(), L.osi_conv_wino_workspace(ctypes.byref(d))
    nb = 2 * v.Pn * Cout * 4                 # [P][C] means then [P][C] M2 (include/osi.h), P = ceil(tiles / 16): not a byte more
    eligible = L.osi_conv_wino_eligible(ctypes.byref(d), 0) == 1
    u = dict(a=torch.zeros(ub // 4), b=torch.zeros(ub // 4))
    if pre and eligible:
        assert ub >= 16 * Cin * Cout * 4 and sb > 0
        for k, vv in (("a", v), ("b", v2)):  # the transformed weights: an output of exactly osi_conv_wino_weights_bytes(d)
            tr = lambda i, o, w: L.osi_conv_wino_transform_weights(ctypes.byref(d), i.w, 0, o.u, ub, T.S())
            u[k] = tt(three_fills(cuda, tr, dict(w=vv.w), dict(w=(v2 if vv is v else v).w), dict(u=((ub // 4,), F32)))[0]["u"])

    def run(i, o, w):
        P, rows = ctypes.c_int(-1), ctypes.c_int(-1)
        tail = (w["ps"].ptr, nb, ctypes.byref(P), ctypes.byref(rows), T.S()) if stats else (None, 0, None, None, T.S())
        if pre:
            rc = L.osi_conv_fwd_wino_pre(ctypes.byref(d), i.x, i.get("sc"), i.get("sh"), i.u, o.y, w["slab"].ptr, w["slab"].nbytes, *tail)
        else:
            rc = L.osi_conv_fwd_wino(ctypes.byref(d), i.x, i.get("sc"), i.get("sh"), i.w, o.y, w["ws"].ptr, w["ws"].nbytes, *tail)
        if rc or not stats:
            return rc
        return rc, dict(ws_out=dict(ps=2 * P.value * Cout), info=dict(P=P.value, rows=rows.value))
    ins = lambda vv, k: dict(x=vv.x, **(dict(u=u[k]) if pre else dict(w=vv.w)), **(dict(sc=vv.sc, sh=vv.sh) if act else {}))
    ws = dict(slab=sb) if pre else dict(ws=wb)
    if stats:
        ws["ps"] = nb
    with T.pinned_knobs(wino_streamk=1):
        r = three_fills(cuda, run, ins(v, "a"), ins(v2, "b"), dict(y=((B, Hh, W, Cout), F32, tile_band(Cout))), ws, band=tile_band(Cout), refusable=not eligible)
    if not eligible:
        assert r is None and shape == WINO[1], "147 tiles: the statistics groups would not hold the same number of pixels"
        return
    assert _slab_touched(r[2], ub) > 0, "the ragged round is meant to be cut along K: its pieces go through the slab"
    ref = v.fwd64(act)
    assert float((tt(r[0]["y"]).double() - ref).abs().max()) <= _bound(Cin * 9, ref)
    if stats:
        assert r[1]["P"] == v.Pn
        _check_group_partials(r[0]["ws:ps"], r[1]["P"], r[1]["rows"], Cout, ref.view(v.M, Cout))


@pytest.mark.parametrize("pre", [False, True], ids=["raw", "pre"])
@pytest.mark.parametrize("act,stats", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("shape", WINO, ids=conv_ids)
def test_wino_forward(cuda, shape, act, stats, pre):
    _wino_fwd_case(cuda, shape, act, stats, pre)


@pytest.mark.parametrize("pre", [False, True], ids=["raw", "pre"])
@pytest.mark.parametrize("partials", [False, True])
@pytest.mark.parametrize("shape", WINO[:2], ids=conv_ids)
def test_wino_input_gradient(cuda, shape, partials, pre):
    L, N, T = _libs()
    B, Hh, W, Cin, Cout = shape
    v, v2 = wino(shape), wino(shape, 1)
    d = v.d
    assert L.osi_conv_wino_eligible(ctypes.byref(d), 1) == 1
    ub, sb, wb = L.osi_conv_wino_weights_bytes(ctypes.byref(d)), L.osi_conv_wino_slab_bytes(), L.osi_conv_wino_workspace(ctypes.byref(d))
    pb = 3 * v.Pn * Cin * 4                  # [3][P][Cin] (include/osi.h), planes 0 and 1 written
    u = {}
    if pre:
        for k, vv in (("a", v), ("b", v2)):
            tr = lambda i, o, w: L.osi_conv_wino_transform_weights(ctypes.byref(d), i.w, 1, o.u, ub, T.S())
            u[k] = tt(three_fills(cuda, tr, dict(w=vv.wd), dict(w=(v2 if vv is v else v).wd), dict(u=((ub // 4,), F32)))[0]["u"])

    def run(i, o, w):
        f = T.Fusion(None, i.y0, i.mean0, i.inv0, None, None, None, w["parts"].ptr if partials else None, pb if partials else 0, i.sc, i.sh)
        P = ctypes.c_int(-1)
        if pre:
            rc = L.osi_conv_dgrad_fused_wino_pre(ctypes.byref(d), i.dy, i.u, o.dx, ctypes.byref(f), w["slab"].ptr, w["slab"].nbytes, ctypes.byref(P), T.S())
        else:
            rc = L.osi_conv_dgrad_fused_wino(ctypes.byref(d), i.dy, i.w, o.dx, ctypes.byref(f), w["ws"].ptr, w["ws"].nbytes, ctypes.byref(P), T.S())
        if rc or not partials:
            return rc
        return rc, dict(ws_out=dict(parts=2 * P.value * Cin), info=dict(P=P.value))
    ins = lambda vv, k: dict(dy=vv.dy, y0=vv.q.y0, mean0=vv.q.mean0, inv0=vv.q.inv0, sc=vv.q.sc, sh=vv.q.sh, **(dict(u=u[k]) if pre else dict(w=vv.wd)))
    ws = dict(slab=sb) if pre else dict(ws=wb)
    if partials:
        ws["parts"] = pb
    with T.pinned_knobs(wino_streamk=1):
        r = three_fills(cuda, run, ins(v, "a"), ins(v2, "b"), dict(dx=((B, Hh, W, Cin), F32, tile_band(Cin))), ws, band=tile_band(Cin))
    assert _slab_touched(r[2], ub) > 0, "the ragged round is meant to be cut along K: its pieces go through the slab"
    ref = v.dgrad64()
    got = tt(r[0]["dx"]).double().view(v.M, Cin)
    assert float((got - ref).abs().max()) <= _bound(Cout * 9, ref)
    assert bool((got[~v.q.gate] == 0).all()), "exact zeros behind a closed gate"
    if partials:
        assert r[1]["P"] == v.Pn
        _check_partial_sums(r[0]["ws:parts"], v.Pn, Cin, ref, [(v.q.y0, v.q.mean0, v.q.inv0)])


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("shape", WINO[:2], ids=conv_ids)
def test_wino_weight_gradient(cuda, shape, act):
    L, N, T = _libs()
    B, Hh, W, Cin, Cout = shape
    v, v2 = wino(shape), wino(shape, 1)
    nb = L.osi_conv_wgrad_wino_workspace(ctypes.byref(v.d))
    assert nb > 0, "the shape is meant to be taken"

    def run(i, o, w):
        return L.osi_conv_wgrad_wino(ctypes.byref(v.d), i.dy, i.x, i.get("sc"), i.get("sh"), o.dw, w["ws"].ptr, w["ws"].nbytes, T.S())
    ins = lambda vv: dict(dy=vv.dy, x=vv.x, **(dict(sc=vv.sc, sh=vv.sh) if act else {}))
    r = three_fills(cuda, run, ins(v), ins(v2), dict(dw=((Cout, 3, 3, Cin), F32, tile_band(Cin))), dict(ws=nb), band=tile_band(64))
    assert _touched(r[2]["ws"]) > 0, "the partial slabs go through the workspace"
    ref = v.wgrad64(act)
    assert float((tt(r[0]["dw"]).double() - ref).abs().max()) <= _bound(v.M, ref)


# ---- stem (csrc/stem_direct.hip, csrc/stem_dgrad.hip) ---------------------------------------------------------------------------------
class _Stem:
    def __init__(self, B, Hh, W, seed=0):
        g = gen("stem", B, Hh, W, seed)
        self.x = torch.rand(B, 3, Hh, W, generator=g)
        self.w = torch.randn(64, 3, 7, 7, generator=g) * 0.05
        self.x4 = torch.zeros(B, Hh, W, 4)
        self.x4[..., :3] = self.x.permute(0, 2, 3, 1)
        self.Hs, self.Ws = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
        self.dy = torch.randn(B, 64, self.Hs, self.Ws, generator=g)
        self.wk = self.w.permute(0, 2, 3, 1).contiguous()                        # [64][7][7][3], the parameter's layout
        self.dyn = self.dy.permute(0, 2, 3, 1).contiguous()
        self.anchor4 = (self.x4 + 0.02 * torch.randn(B, Hh, W, 4, generator=g)).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def stem(B, Hh, W, seed=0):
    return _Stem(B, Hh, W, seed)


@pytest.mark.parametrize("B,Hh", [(2, 32), (3, 45)])
def test_stem_forward(cuda, B, Hh):
    """The stem through osi_conv_fwd on the NHWC4 image and packed weights: 32 x 32, and 45 x 45 (the generic path)."""
    L, N, T = _libs()
    s, s2 = stem(B, Hh, Hh), stem(B, Hh, Hh, 1)
    d = N.ConvDesc.make(B, Hh, Hh, 4, 64, 7, 2, 3)

    def packed(v):      # osi_stem_weight_pack, guarded as well: [64][224]
        run = lambda i, o, w: L.osi_stem_weight_pack(i.w, o.wp, 64, T.S())
        return tt(three_fills(cuda, run, dict(w=v.wk), dict(w=(s2 if v is s else s).wk), dict(wp=((64, 224), F32)))[0]["wp"])
    run = lambda i, o, w: L.osi_conv_fwd(ctypes.byref(d), i.x4, i.wp, o.y, 0, T.S())
    r = three_fills(cuda, run, dict(x4=s.x4, wp=packed(s)), dict(x4=s2.x4, wp=packed(s2)), dict(y=((B, d.Ho, d.Wo, 64), F32, tile_band(64))))
    ref = lambda dt: F.conv2d(s.x.to(dt), s.w.to(dt), None, 2, 3).permute(0, 2, 3, 1)
    _check_vs64(tt(r[0]["y"]), ref(F32), ref(torch.float64), "stem fwd")


def test_stem_weight_gradient_direct(cuda):
    """B = 2, 64 x 64: the smallest geometry the direct form takes (Ho = Wo = 32); one partial per workgroup through the workspace."""
    L, N, T = _libs()
    B, Hh = 2, 64
    s, s2 = stem(B, Hh, Hh), stem(B, Hh, Hh, 1)
    d = N.ConvDesc.make(B, Hh, Hh, 4, 64, 7, 2, 3)
    nb = L.osi_stem_wgrad_direct_workspace(ctypes.byref(d))
    assert nb > 0
    run = lambda i, o, w: L.osi_stem_wgrad_direct(ctypes.byref(d), i.dy, i.x4, o.dw, w["ws"].ptr, w["ws"].nbytes, T.S())
    r = three_fills(cuda, run, dict(dy=s.dyn, x4=s.x4), dict(dy=s2.dyn, x4=s2.x4), dict(dw=((64, 7, 7, 3), F32)), dict(ws=nb), band=tile_band(64))
    assert _touched(r[2]["ws"]) > 0
    ref = torch.nn.grad.conv2d_weight(s.x.double(), (64, 3, 7, 7), s.dy.double(), 2, 3).permute(0, 2, 3, 1)
    assert float((tt(r[0]["dw"]).double() - ref).abs().max()) <= _bound(B * d.Ho * d.Wo, ref)      # tests/test_stem_tail_gpu.py


def test_stem_weight_gradient_fused_tail(cuda):
    """osi_stem_wgrad_fused at B = 2, 64 x 64: against the fp64 evaluation of the same mathematics on the stored arg-max bytes, under
    the bounds of tests/test_stem_tail_gpu.py (rel-L2 5e-5, max 2e-4 of the scale)."""
    L, N, T = _libs()
    B, Hh, C = 2, 64, 64
    d = N.ConvDesc.make(B, Hh, Hh, 4, 64, 7, 2, 3)
    Ho, Hp = d.Ho, (d.Ho + 2 - 3) // 2 + 1
    M = B * Ho * Ho
    nb, wsb = L.osi_stem_wgrad_fused_workspace(ctypes.byref(d)), L.osi_bn_backward_workspace(M, C)
    assert nb > 0

    def setup(seed):
        s = stem(B, Hh, Hh, seed)
        g = gen("stem-fused", seed)
        y = F.conv2d(s.x, s.w, None, 2, 3).permute(0, 2, 3, 1).contiguous()
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        v = y.double().view(M, C)
        mean, inv = v.mean(0).float(), (1 / torch.sqrt(v.var(0, unbiased=False) + 1e-5)).float()
        scale = gamma * inv
        gpool = torch.randn(B, Hp, Hp, C, generator=g)
        yd, scd, shd, gpd, md, ivd, gad = (t.to(cuda) for t in (y, scale, beta - mean * scale, gpool, mean, inv, gamma))
        pooled, idx = torch.empty(B, Hp, Hp, C, device=cuda), torch.zeros(B * Hp * Hp * C, dtype=U8, device=cuda)
        N.check(L.osi_bn_relu_maxpool_fwd(N.ptr(yd), N.ptr(scd), N.ptr(shd), N.ptr(pooled), N.ptr(idx), B, Ho, Ho, C, T.S()))
        dg, db, ws = torch.empty(C, device=cuda), torch.empty(C, device=cuda), torch.empty(wsb, dtype=U8, device=cuda)
        N.check(L.osi_bn_relu_maxpool_bwd(N.ptr(gpd), N.ptr(idx), N.ptr(yd), N.ptr(md), N.ptr(ivd), N.ptr(gad), None, N.ptr(dg), N.ptr(db), B, Ho, Ho, C,
                                          N.ptr(ws), wsb, T.S()))
        torch.cuda.synchronize()
        return dict(gpool=gpool, idx=idx.cpu(), y=y, x4=s.x4, gamma=gamma, mean=mean, inv=inv, dg=dg.cpu(), db=db.cpu()), s
    (a, s), (a2, _) = setup(0), setup(1)
    run = lambda i, o, w: L.osi_stem_wgrad_fused(ctypes.byref(d), i.gpool, i.idx, i.y, i.x4, i.gamma, i.mean, i.inv, i.dg, i.db, o.dw, w["ws"].ptr, w["ws"].nbytes, T.S())
    r = three_fills(cuda, run, a, a2, dict(dw=((64, 7, 7, 3), F32)), dict(ws=nb), band=tile_band(64))
    assert _touched(r[2]["ws"]) > 0
    ib = a["idx"].view(B, Hp, Hp, C).long()
    gate, tap = ib >= 128, ib % 128
    hh = (torch.arange(Hp).view(1, -1, 1, 1) * 2 - 1 + tap // 3).clamp(0, Ho - 1)
    ww = (torch.arange(Hp).view(1, 1, -1, 1) * 2 - 1 + tap % 3).clamp(0, Ho - 1)
    bb, cc = torch.arange(B).view(-1, 1, 1, 1).expand_as(ib), torch.arange(C).view(1, 1, 1, -1).expand_as(ib)
    g64 = torch.zeros(B, Ho, Ho, C, dtype=torch.float64)
    g64.index_put_((bb, hh, ww, cc), a["gpool"].double() * gate.double(), accumulate=True)
    xh = (a["y"].double() - a["mean"].double()) * a["inv"].double()
    c1, c2 = g64.view(M, C).mean(0), (g64 * xh).view(M, C).mean(0)
    dy64 = (g64 - c1 - xh * c2) * (a["gamma"].double() * a["inv"].double())
    dw64 = torch.nn.grad.conv2d_weight(s.x.double(), (64, 3, 7, 7), dy64.permute(0, 3, 1, 2), 2, 3).permute(0, 2, 3, 1)
    got = tt(r[0]["dw"]).double()
    assert float((got - dw64).norm() / dw64.norm()) <= 5e-5 and float((got - dw64).abs().max()) <= 2e-4 * float(dw64.abs().max())


def _stem_dx64(s):
    return torch.nn.grad.conv2d_input(tuple(s.x.shape), s.w.double(), s.dy.double(), stride=2, padding=3)


@pytest.mark.parametrize("B,Hh,W", [(2, 32, 32), (2, 33, 39)])
def test_stem_input_gradient(cuda, B, Hh, W):
    L, N, T = _libs()
    s, s2 = stem(B, Hh, W), stem(B, Hh, W, 1)
    run = lambda i, o, w: L.osi_stem_dgrad(i.dy, i.w, o.dx, B, Hh, W, T.S())
    r = three_fills(cuda, run, dict(dy=s.dyn, w=s.wk), dict(dy=s2.dyn, w=s2.wk), dict(dx=((B, 3, Hh, W), F32)))
    ref = _stem_dx64(s)
    assert float((tt(r[0]["dx"]).double() - ref).abs().max()) <= (2e-6 + 6e-8 * math.sqrt(64 * 49)) * float(ref.abs().max())    # tests/test_input_grad_gpu.py


@pytest.mark.parametrize("attack", ["fgsm", "pgd"])
def test_stem_input_gradient_attack_epilogues(cuda, attack):
    """osi_stem_dgrad_fgsm / _pgd at 2 x 33 x 39: the fp64 gradient's choice in every pixel whose |dx| is above the kernel's own error
    bound, and at most 1e-4 of the pixels below it (tests/test_adversarial_gpu.py, tests/test_pgd_gpu.py)."""
    L, N, T = _libs()
    B, Hh, W, eps, alpha = 2, 33, 39, 8 / 255, 2 / 255
    s, s2 = stem(B, Hh, W), stem(B, Hh, W, 1)

    def run(i, o, w):
        if attack == "fgsm":
            return L.osi_stem_dgrad_fgsm(i.dy, i.w, i.x4, o.out, eps, 0.0, 1.0, B, Hh, W, T.S())
        return L.osi_stem_dgrad_pgd(i.dy, i.w, i.x4, i.a4, o.out, alpha, eps, 0.0, 1.0, B, Hh, W, T.S())
    ins = lambda v: dict(dy=v.dyn, w=v.wk, x4=v.x4, **(dict(a4=v.anchor4) if attack == "pgd" else {}))
    r = three_fills(cuda, run, ins(s), ins(s2), dict(out=((B, Hh, W, 4), F32)))
    ref = _stem_dx64(s)
    excluded = (ref.abs() <= (2e-6 + 6e-8 * math.sqrt(64 * 49)) * float(ref.abs().max())).permute(0, 2, 3, 1)
    sgn = torch.sign(ref).float().permute(0, 2, 3, 1)
    x = s.x4[..., :3]
    if attack == "fgsm":
        twin = torch.clamp(x + eps * sgn, 0.0, 1.0)
    else:
        a = s.anchor4[..., :3]
        twin = torch.clamp(torch.min(torch.max(x + alpha * sgn, a - eps), a + eps), 0.0, 1.0)
    got = tt(r[0]["out"])
    assert bool((got[..., 3] == 0).all())
    assert int(((got[..., :3] != twin) & ~excluded).sum()) == 0 and float(excluded.double().mean()) <= 1e-4


# ---- pools and layout (csrc/pool_layout.hip, the stem tail of csrc/bn.hip) ---------------------------------------------------------------
POOL = [(2, 17, 23, 64), (4, 9, 9, 8)]


class _Pool:
    def __init__(self, shape, seed=0):
        B, Hh, W, C = shape
        g = gen("pool", shape, seed)
        self.Ho, self.Wo = (Hh - 1) // 2 + 1, (W - 1) // 2 + 1
        self.y = torch.randn(B, Hh, W, C, generator=g) * 2 + 0.3
        self.y[0, :4, :4] = -5.0                 # a window whose maximum is not positive
        self.x = torch.relu(self.y)              # post-ReLU input of the plain pool: many exact ties at 0
        self.gamma, self.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        v = self.y.double().view(-1, C)
        self.mean, self.inv = v.mean(0).float(), (1 / torch.sqrt(v.var(0, unbiased=False) + 1e-5)).float()
        self.scale = self.gamma * self.inv
        self.shift = self.beta - self.mean * self.scale
        self.gp = torch.randn(B, self.Ho, self.Wo, C, generator=g)
        # the activation the fused forward pools, with the kernels' roundings (one fma, one max), and torch's pool of it
        self.a = torch.relu(torch.addcmul(self.shift.double(), self.y.double(), self.scale.double()).float())


@functools.lru_cache(maxsize=None)
def pool(shape, seed=0):
    return _Pool(shape, seed)


def _maxpool_ref(a, gp):
    """torch's max-pool of a (NHWC), its arg-max as tap 0..8 of the 3x3 window, and its backward of gp (first-max tie rule)."""
    B, Hh, W, C = a.shape
    t = a.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y, idx = F.max_pool2d(t, 3, 2, 1, return_indices=True)
    y.backward(gp.permute(0, 3, 1, 2))
    ho, wo = torch.arange(y.shape[2]).view(1, 1, -1, 1), torch.arange(y.shape[3]).view(1, 1, 1, -1)
    tap = (idx // W - (2 * ho - 1)) * 3 + (idx % W - (2 * wo - 1))
    return y.detach().permute(0, 2, 3, 1), tap.permute(0, 2, 3, 1), t.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", POOL, ids=conv_ids)
def test_maxpool_forward_backward(cuda, shape):
    L, N, T = _libs()
    B, Hh, W, C = shape
    p, p2 = pool(shape), pool(shape, 1)
    oshape = (B, p.Ho, p.Wo, C)
    run = lambda i, o, w: L.osi_maxpool3x3s2_fwd(i.x, o.y, o.idx, B, Hh, W, C, T.S())
    r = three_fills(cuda, run, dict(x=p.x), dict(x=p2.x), dict(y=(oshape, F32), idx=((B * p.Ho * p.Wo * C,), U8)))
    y, tap, dx = _maxpool_ref(p.x, p.gp)
    assert torch.equal(tt(r[0]["y"]), y), "exact, as tests/test_kernels_gpu.py::test_maxpool"
    idx = tt(r[0]["idx"]).view(oshape).long()
    assert torch.equal(idx, tap), "arg-max bytes: torch's first maximum"
    run = lambda i, o, w: L.osi_maxpool3x3s2_bwd(i.dy, i.idx, o.dx, B, Hh, W, C, T.S())
    rb = three_fills(cuda, run, dict(dy=p.gp, idx=tt(r[0]["idx"])), dict(dy=p2.gp, idx=tt(r[0]["idx"])), dict(dx=((B, Hh, W, C), F32)))
    assert torch.allclose(tt(rb[0]["dx"]), dx, atol=1e-6)


@pytest.mark.parametrize("shape", POOL, ids=conv_ids)
def test_stem_tail_forward_backward(cuda, shape):
    """osi_bn_relu_maxpool_fwd, _bwd and _bwd_frozen: pooled activation and arg-max bytes exact against torch's pool of the activation
    with the kernel's roundings; the backward against fp64 through the stored bytes (bounds of tests/test_frozen_bn_gpu.py)."""
    from test_frozen_bn_gpu import _bound as frozen_bound
    L, N, T = _libs()
    B, Hh, W, C = shape
    p, p2 = pool(shape), pool(shape, 1)
    M = B * Hh * W
    oshape = (B, p.Ho, p.Wo, C)
    run = lambda i, o, w: L.osi_bn_relu_maxpool_fwd(i.y, i.scale, i.shift, o.pooled, o.idx, B, Hh, W, C, T.S())
    fwd = lambda v: three_fills(cuda, run, dict(y=v.y, scale=v.scale, shift=v.shift), dict(y=(p2 if v is p else p).y, scale=v.shift, shift=v.scale),
                                dict(pooled=(oshape, F32), idx=((B * p.Ho * p.Wo * C,), U8)))[0]
    f1, f2 = fwd(p), fwd(p2)
    y, tap, _ = _maxpool_ref(p.a, p.gp)
    assert torch.equal(tt(f1["pooled"]), y)
    idx = tt(f1["idx"]).view(oshape).long()
    assert torch.equal(idx & 0x7F, tap) and torch.equal(idx >> 7, (y > 0).long()), "tap, and bit 7 = window maximum > 0"
    assert bool((idx >> 7 == 0).any()) and bool((idx >> 7 == 1).any())
    # fp64 through the stored bytes: scatter of the bit-7-gated gradient, then the BatchNorm backward
    g64 = torch.zeros(B, Hh, W, C, dtype=torch.float64)
    hh = (torch.arange(p.Ho).view(1, -1, 1, 1) * 2 - 1 + (idx & 0x7F) // 3).clamp(0, Hh - 1)
    ww = (torch.arange(p.Wo).view(1, 1, -1, 1) * 2 - 1 + (idx & 0x7F) % 3).clamp(0, W - 1)
    bb, cc = torch.arange(B).view(-1, 1, 1, 1).expand_as(idx), torch.arange(C).view(1, 1, 1, -1).expand_as(idx)
    g64.index_put_((bb, hh, ww, cc), p.gp.double() * (idx >> 7).double(), accumulate=True)
    gv = g64.view(M, C)
    xh = (p.y.double().view(M, C) - p.mean.double()) * p.inv.double()
    db, dg = gv.sum(0), (gv * xh).sum(0)
    nb = L.osi_bn_backward_workspace(M, C)
    for frozen in (False, True):
        def run(i, o, w):
            f = L.osi_bn_relu_maxpool_bwd_frozen if frozen else L.osi_bn_relu_maxpool_bwd
            return f(i.gp, i.idx, i.y, i.mean, i.inv, i.scale if frozen else i.gamma, o.dy, o.dg, o.db, B, Hh, W, C, w["ws"].ptr, w["ws"].nbytes, T.S())
        ins = lambda v, f: dict(gp=v.gp, idx=tt(f["idx"]), y=v.y, mean=v.mean, inv=v.inv, gamma=v.gamma, scale=v.scale)
        for merge in (False, True):
            with _knobs(T, merge):
                r = three_fills(cuda, run, ins(p, f1), ins(p2, f2), dict(dy=((B, Hh, W, C), F32, tile_band(C)), dg=((C,), F32), db=((C,), F32)), dict(ws=nb))
            assert _touched(r[2]["ws"]) > 0
            ref = gv * p.scale.double() if frozen else p.gamma.double() * p.inv.double() * (gv - db / M - xh * dg / M)
            got = tt(r[0]["dy"]).double().view(M, C)
            if frozen:
                assert float((got - ref).abs().max()) <= frozen_bound(4, ref) and bool((got[gv == 0] == 0).all())
            else:
                _check_vs64(got, ref.float(), ref, "stem tail dy", **BWD)
            for name, want in (("dg", dg), ("db", db)):
                if frozen:
                    assert float((tt(r[0][name]).double() - want).abs().max()) <= frozen_bound(M, want), name
                else:
                    _check_vs64(tt(r[0][name]), want.float(), want, name, **BWD)


@pytest.mark.parametrize("B,HW,C", [(3, 49, 2048), (5, 9, 12)])
def test_avgpool(cuda, B, HW, C):
    L, N, T = _libs()
    g, g2 = gen("avg", B, HW, C), gen("avg2", B, HW, C)
    x, dy, x2, dy2 = torch.randn(B, HW, C, generator=g), torch.randn(B, C, generator=g), torch.randn(B, HW, C, generator=g2), torch.randn(B, C, generator=g2)
    r = three_fills(cuda, lambda i, o, w: L.osi_avgpool_fwd(i.x, o.y, B, HW, C, T.S()), dict(x=x), dict(x=x2), dict(y=((B, C), F32)))
    assert torch.allclose(tt(r[0]["y"]), x.mean(1), atol=1e-6), "the bound of tests/test_kernels_gpu.py::test_avgpool"
    r = three_fills(cuda, lambda i, o, w: L.osi_avgpool_bwd(i.dy, o.dx, B, HW, C, T.S()), dict(dy=dy), dict(dy=dy2), dict(dx=((B, HW, C), F32)))
    assert torch.allclose(tt(r[0]["dx"]), (dy / HW).view(B, 1, C).expand(B, HW, C), atol=1e-7)


def test_layout_conversions(cuda):
    """osi_nchw3_to_nhwc4, osi_u8hwc3_to_nhwc4, osi_u8_crop_flip_to_nhwc4 at B = 3, canvas 37 x 41, crop 32 x 32: exact against numpy.
    The canvas sits in a halo of 255s: a corner the kernel does not clamp reads them."""
    L, N, T = _libs()
    B, Hc, Wc, Hh, W = 3, 37, 41, 32, 32
    g, g2 = gen("layout"), gen("layout2")
    x, x2 = torch.rand(B, 3, Hc, Wc, generator=g), torch.rand(B, 3, Hc, Wc, generator=g2)
    r = three_fills(cuda, lambda i, o, w: L.osi_nchw3_to_nhwc4(i.x, o.y, B, Hc, Wc, T.S()), dict(x=x), dict(x=x2), dict(y=((B, Hc, Wc, 4), F32)))
    assert torch.equal(tt(r[0]["y"])[..., :3], x.permute(0, 2, 3, 1)) and float(tt(r[0]["y"])[..., 3].abs().max()) == 0
    can, can2 = (torch.randint(0, 255, (B, Hc, Wc, 3), generator=gg, dtype=U8) for gg in (g, g2))     # 0 .. 254: a 255 is the halo's
    flip, noflip = torch.tensor([1, 0, 1], dtype=U8), torch.zeros(3, dtype=U8)
    to_f = lambda u8: np.concatenate([u8.numpy().astype(np.float32) / np.float32(255), np.zeros(u8.shape[:-1] + (1,), np.float32)], axis=-1)
    r = three_fills(cuda, lambda i, o, w: L.osi_u8hwc3_to_nhwc4(i.x, i.flip, o.y, B, Hc, Wc, T.S()), dict(x=can, flip=flip), dict(x=can2, flip=noflip),
                    dict(y=((B, Hc, Wc, 4), F32)))
    want = to_f(can)
    want[[0, 2]] = want[[0, 2], :, ::-1]
    assert H.same_bytes(r[0]["y"], np.ascontiguousarray(want))
    # corners (x0, y0): (0, 0), the far corner, and one out of range on both axes that the kernel clamps to the far / near edge
    for corners in ([(0, 0), (Wc - W, Hc - Hh), (Wc + 5, -3)], [(3, 2), (-7, Hc), (Wc - W, 0)]):
        xy = torch.tensor(corners, dtype=I32)
        run = lambda i, o, w: L.osi_u8_crop_flip_to_nhwc4(i.x, i.xy, i.flip, o.y, B, Hc, Wc, Hh, W, T.S())
        r = three_fills(cuda, run, dict(x=can, xy=xy, flip=flip), dict(x=can2, xy=xy.flip(0).contiguous(), flip=noflip), dict(y=((B, Hh, W, 4), F32)))
        want = np.zeros((B, Hh, W, 4), np.float32)
        for b, (x0, y0) in enumerate(corners):
            x0, y0 = min(max(x0, 0), Wc - W), min(max(y0, 0), Hc - Hh)
            crop = to_f(can[b, y0:y0 + Hh, x0:x0 + W])
            want[b] = crop[:, ::-1] if int(flip[b]) else crop
        assert H.same_bytes(r[0]["y"], want), corners
        assert float(r[0]["y"].max()) < 1.0, "a 255 of the halo was read"


# ---- head, losses, optimizer (csrc/linear.hip, csrc/loss.hip, csrc/optim.hip) --------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("B,K,O", [(7, 30, 30), (5, 2048, 116)])
def test_linear(cuda, B, K, O, bias):
    L, N, T = _libs()

    def draw(seed):
        g = gen("linear", B, K, O, seed)
        return dict(x=torch.randn(B, K, generator=g), w=torch.randn(O, K, generator=g) / K ** .5, b=torch.randn(O, generator=g), dy=torch.randn(B, O, generator=g),
                    base=torch.randn(B, K, generator=g))
    v, v2 = draw(0), draw(1)

    def ref(dt):
        xx, ww, bb = (v[k].to(dt).clone().requires_grad_(True) for k in ("x", "w", "b"))
        y = F.linear(xx, ww, bb if bias else None)
        y.backward(v["dy"].to(dt))
        return y.detach(), xx.grad, ww.grad, bb.grad if bias else None
    r32, r64 = ref(F32), ref(torch.float64)
    run = lambda i, o, w: L.osi_linear_fwd(i.x, i.w, i.b, o.y, B, K, O, T.S())
    ins = lambda d: dict(x=d["x"], w=d["w"], b=d["b"] if bias else None)
    r = three_fills(cuda, run, ins(v), ins(v2), dict(y=((B, O), F32)))
    _check_vs64(tt(r[0]["y"]), r32[0], r64[0], "linear fwd")
    for acc in (0, 1):
        run = lambda i, o, w: L.osi_linear_bwd(i.dy, i.x, i.w, o.dx, acc, o.dw, o.get("db"), B, K, O, T.S())
        ins = lambda d: dict(dy=d["dy"], x=d["x"], w=d["w"])
        outs = dict(dx=v["base"] if acc else ((B, K), F32), dw=((O, K), F32), **(dict(db=((O,), F32)) if bias else {}))
        r = three_fills(cuda, run, ins(v), ins(v2), outs)
        _check_vs64(tt(r[0]["dx"]), r32[1] + (v["base"] if acc else 0), r64[1] + (v["base"].double() if acc else 0), f"linear dx accumulate {acc}")
        _check_vs64(tt(r[0]["dw"]), r32[2], r64[2], "linear dw")
        if bias:
            _check_vs64(tt(r[0]["db"]), r32[3], r64[3], "linear db")


@pytest.mark.parametrize("mode", ["entropic", "softmax", "garbage", "objectosphere"])
def test_loss_forward_backward(cuda, mode):
    """osi_loss_fwd_bwd in its three modes and with the objectosphere term at (B, C, F) = (17, 65, 30), against the oracle's losses in
    fp64 under the bounds of tests/test_kernels_gpu.py (golden and objectosphere tests)."""
    from oracle import losses_oracle as LO
    L, N, T = _libs()
    B, C, Fd = 17, 65, 30
    m = dict(entropic=N.LOSS_ENTROPIC, softmax=N.LOSS_SOFTMAX, garbage=N.LOSS_GARBAGE, objectosphere=N.LOSS_ENTROPIC)[mode]
    Cz = C + 1 if mode == "garbage" else C           # the garbage class is one more logit column

    def draw(seed):
        g = gen("loss", mode, seed)
        y = torch.randint(-1, C, (B,), generator=g)
        y[0], y[1] = -1, C - 1
        d = dict(z=torch.randn(B, Cz, generator=g) * 2, y=y, f=torch.randn(B, Fd, generator=g) * 3, cw=torch.rand(Cz, generator=g) + 0.5)
        d["f"][2] = 0                                # |f| = 0: gradient defined as 0
        return d
    v, v2 = draw(0), draw(1)
    obj, w, xi, alpha = mode == "objectosphere", 0.5, 3.0, 0.5

    def run(i, o, w_):
        return L.osi_loss_fwd_bwd(m, i.z, i.y, B, Cz, w if m == N.LOSS_ENTROPIC else 1.0, -1, i.get("cw"), i.get("f"), Fd if obj else 0, xi if obj else 0.0,
                                  alpha if obj else 0.0, o.loss, o.dz, o.get("df"), T.S())

    def ins(d):
        yy = d["y"].clone()
        if mode == "garbage":
            yy[yy < 0] = C                           # unknowns are the last class
        return dict(z=d["z"], y=yy, **(dict(cw=d["cw"]) if mode == "garbage" else {}), **(dict(f=d["f"]) if obj else {}))
    r = three_fills(cuda, run, ins(v), ins(v2), dict(loss=((1,), F32), dz=((B, Cz), F32), **(dict(df=((B, Fd), F32)) if obj else {})))
    z64, f64 = v["z"].double().requires_grad_(True), v["f"].double().requires_grad_(True)
    if mode == "entropic":
        J = LO.entropic_openset_loss(z64, v["y"], w)
    elif obj:
        J = LO.objectosphere_loss(z64, v["y"], f64, w, xi, alpha)
    elif mode == "softmax":
        J = F.cross_entropy(z64, v["y"], ignore_index=-1)
    else:
        J = F.cross_entropy(z64, ins(v)["y"], weight=v["cw"].double())
    J.backward()
    assert abs(float(r[0]["loss"][0]) - float(J.detach())) <= 2e-6 * max(1.0, abs(float(J.detach())))
    tol = 2e-7 + 1e-6 * float(z64.grad.abs().max()) + 2e-8 * float(v["z"].abs().max())
    assert float((tt(r[0]["dz"]).double() - z64.grad).abs().max()) <= tol
    if obj:
        want = torch.nan_to_num(f64.grad)
        assert float((tt(r[0]["df"]).double() - want).abs().max()) < 1e-6 * max(1.0, float(want.abs().max()))


def test_softmax(cuda):
    L, N, T = _libs()
    z, z2 = torch.randn(17, 65, generator=gen("sm")) * 4, torch.randn(17, 65, generator=gen("sm2")) * 4
    r = three_fills(cuda, lambda i, o, w: L.osi_softmax(i.z, o.out, 17, 65, T.S()), dict(z=z), dict(z=z2), dict(out=((17, 65), F32)))
    assert torch.allclose(tt(r[0]["out"]), torch.softmax(z.double(), 1).float(), atol=1e-7, rtol=1e-5), "tests/test_kernels_gpu.py::test_softmax_kernel"


def _arena(n, seed):
    g = gen("optim", n, seed)
    return dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g) * 0.3, m=torch.randn(n, generator=g) * 0.1, v=torch.rand(n, generator=g) * 0.01)


@pytest.mark.parametrize("n", [1000, 4100])
@pytest.mark.parametrize("kind", ["adam", "sgd", "adam_groups", "sgd_groups", "adam_groups_dev", "sgd_groups_dev", "accumulate"])
def test_optimizer_steps(cuda, n, kind):
    """The fused steps (Adam and SGD; with groups: plain Adam + AdamW, plain SGD + Nesterov with weight decay; the `_dev` forms of the
    grouped steps with the gradient scale 0.75 read from device memory: the bits of the host-scalar form called with 0.75) at n = 1000
    and 4100 (250 and 1025 units of 16 bytes: no multiple of a 256-unit tile). The issue's 4099 is no multiple of 4: every entry point here refuses it before a launch (asserted below, bands whole, nothing written), 4100 is the
    nearest size the header accepts. State buffers are read and written: uploaded with their bits. Bound: 1e-6 on the parameters as
    tests/test_kernels_gpu.py::test_adam_sgd_vs_torch, against torch's own single-tensor step."""
    L, N, T = _libs()
    a, a2 = _arena(n, 0), _arena(n, 1)
    lr, step = 1e-2, 3
    dev_form = kind.endswith("_dev")
    gs = 0.75 if dev_form else 1.0

    def launcher(n, dev_form=dev_form):
        segs = (N.OptSegment * 2)(N.OptSegment(0, n // 8, 0), N.OptSegment(n // 8 + 1, n // 4, 1))       # unit n/8 belongs to no group
        ag = (N.AdamGroup * 2)(N.AdamGroup(lr, 0.9, 0.999, 1e-8, 0.0, step, 0, 0, 0), N.AdamGroup(lr, 0.9, 0.999, 1e-8, 0.05, step, 1, 0, 0))
        sg = (N.SgdGroup * 2)(N.SgdGroup(lr, 0.9, 0.0, 0.0, 0, 0, 0), N.SgdGroup(lr, 0.9, 0.0, 0.05, 1, 0, 0))

        def run(i, o, w):
            if kind == "adam":
                return L.osi_adam_step(o.p, i.g, o.m, o.v, n, lr, 0.9, 0.999, 1e-8, step, 1.0, T.S())
            if kind == "sgd":
                return L.osi_sgd_step(o.p, i.g, o.m, n, lr, 0.9, 0, 1.0, T.S())
            if kind.startswith("adam_groups"):
                if dev_form:
                    return L.osi_adam_step_groups_dev(o.p, i.g, o.m, o.v, None, n, segs, 2, ag, 2, i.gs, T.S())
                return L.osi_adam_step_groups(o.p, i.g, o.m, o.v, None, n, segs, 2, ag, 2, gs, T.S())
            if kind.startswith("sgd_groups"):
                if dev_form:
                    return L.osi_sgd_step_groups_dev(o.p, i.g, o.m, n, segs, 2, sg, 2, i.gs, T.S())
                return L.osi_sgd_step_groups(o.p, i.g, o.m, n, segs, 2, sg, 2, gs, T.S())
            return L.osi_grad_accumulate(o.p, i.g, n, T.S())
        return run
    ins = lambda d: dict(g=d["g"], **(dict(gs=torch.tensor([gs])) if dev_form else {}))
    outs = lambda d: dict(p=d["p"], **(dict(m=d["m"]) if kind != "accumulate" else {}), **(dict(v=d["v"]) if "adam" in kind else {}))
    if n == 4100:      # the refused size first: 4099 floats
        bad = {k: t[:4099].contiguous() for k, t in a.items()}
        assert _once(cuda, launcher(4099), ins(bad), outs(bad), {}, refusable=True) is None, "n % 4 != 0 is refused"
    r = three_fills(cuda, launcher(n), ins(a), ins(a2), outs(a))
    if dev_form:
        host = three_fills(cuda, launcher(n, False), ins(a), ins(a2), outs(a))
        assert all(H.same_bits_nan(r[0][k], host[0][k]) for k in r[0]), "the scalar from device memory: the bits of the host-scalar step"

    def torch_step(lo, hi, opt):
        pt = a["p"][lo:hi].clone().requires_grad_(True)
        pt.grad = a["g"][lo:hi] * gs             # the kernels scale the gradient first: one fp32 rounding, exact at 1.0
        o = opt([pt])
        st = o.state[pt]
        if "adam" in kind:
            st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(float(step - 1)), a["m"][lo:hi].clone(), a["v"][lo:hi].clone()
        else:
            st["momentum_buffer"] = a["m"][lo:hi].clone()
        o.step()
        return pt.detach()
    cut = 4 * (n // 8)
    adam = lambda **kw: (lambda ps: torch.optim.Adam(ps, lr=lr, foreach=False, **kw))
    adamw = lambda ps: torch.optim.AdamW(ps, lr=lr, weight_decay=0.05, foreach=False)
    sgd = lambda **kw: (lambda ps: torch.optim.SGD(ps, lr=lr, momentum=0.9, foreach=False, **kw))
    got = tt(r[0]["p"])
    if kind == "accumulate":
        assert torch.equal(got, a["p"] + a["g"]), "one fp32 add per element"
        return
    if kind in ("adam", "sgd"):
        want = torch_step(0, n, adam() if kind == "adam" else sgd())
    else:
        first = torch_step(0, cut, adam() if "adam" in kind else sgd())
        second = torch_step(cut + 4, n, adamw if "adam" in kind else sgd(weight_decay=0.05, nesterov=True))
        want = torch.cat([first, a["p"][cut:cut + 4], second])
        assert torch.equal(got[cut:cut + 4], a["p"][cut:cut + 4]) and torch.equal(tt(r[0]["m"])[cut:cut + 4], a["m"][cut:cut + 4])
    assert float((got - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("n", [1000, 4100])
@pytest.mark.parametrize("norm", ["l2", "inf"])
def test_grad_clip_scale(cuda, n, norm):
    """osi_grad_clip_scale with a workspace of exactly osi_grad_norm_workspace(n), over the whole arena and over spans whose last one
    has numel % 4 != 0. Bounds of tests/test_grad_clip_gpu.py: the norm within 2^-22 of the fp64 value, the scalar within 1 ulp."""
    L, N, T = _libs()
    a, a2 = _arena(n, 0), _arena(n, 1)
    nb = L.osi_grad_norm_workspace(n)
    assert nb > 0 and nb % 8 == 0
    nt = N.NORM_L2 if norm == "l2" else N.NORM_INF
    if n == 4100:      # 4099 floats: no workspace size, and the call is refused before any launch (bands whole, out2 untouched)
        assert L.osi_grad_norm_workspace(4099) == 0
        bad = lambda i, o, w: L.osi_grad_clip_scale(i.g, 4099, None, 0, nt, 0.5, 1.0, w["ws"].ptr, w["ws"].nbytes, o.out2, T.S())
        assert _once(cuda, bad, dict(g=a["g"][:4099].contiguous()), dict(out2=((2,), F32)), dict(ws=H.Ws(nb, cuda)), refusable=True) is None
    spans = (N.GradSpan * 2)(N.GradSpan(0, 13), N.GradSpan(16, n - 16 - 1))
    for use_spans in (False, True):
        run = lambda i, o, w: L.osi_grad_clip_scale(i.g, n, spans if use_spans else None, 2 if use_spans else 0, nt, 0.5, 1.0, w["ws"].ptr, w["ws"].nbytes, o.out2, T.S())
        r = three_fills(cuda, run, dict(g=a["g"]), dict(g=a2["g"]), dict(out2=((2,), F32)), dict(ws=nb))
        assert _touched(r[2]["ws"]) > 0
        g = a["g"].double()
        if use_spans:
            g = torch.cat([g[:13], g[16:n - 1]])
        want = 0.5 * (float(g.norm()) if norm == "l2" else float(g.abs().max()))
        assert abs(float(r[0]["out2"][0]) - want) <= 2.0 ** -22 * want
        coef = np.float32(0.5) * min(np.float32(1), np.float32(1) / (r[0]["out2"][0] + np.float32(1e-6)) * np.float32(1.0))
        assert H.ulps(r[0]["out2"][1:], np.float32([coef])) <= 1

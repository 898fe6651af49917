"""NaN and Inf propagate through every kernel like through torch (include/osi.h, conventions; DESIGN.md, divergences): the set of
non-finite output elements of an entry point equals that of the torch fp64 reference of the same operation, and every finite element
stays within the bound the parity test of that entry point uses (imported from that test, not restated). NaN versus +-Inf is not
asserted, nor a non-finite value times a structural zero, which NaN of a window the arg-max names, or the backward gate of a NaN
activation. Cases and references: tests/nonfinite_cases.py (anchored without a kernel by tests/test_nonfinite_cpu.py).

Every call goes through the C ABI, and every output buffer starts filled with a finite sentinel, so that an element a kernel never
wrote cannot look like propagation."""
import ctypes

import pytest
import torch

import nonfinite_cases as NF
from test_head_kernels_gpu import _check_dlogits, _check_loss
from test_kernels_gpu import _check_vs64
from test_production_shapes_gpu import _bound

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
F32, F64 = torch.float32, torch.float64


def _full(shape, cuda, dtype=torch.float32):
    return torch.full(tuple(shape), SENTINEL, device=cuda, dtype=dtype)


def _same(got, ref32, ref64, what, check=_check_vs64, **kw):
    """THE comparison: equal non-finite sets, then the parity test's bound on the finite elements (both sides 0 elsewhere)."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref64.shape)}"
    bad, bad_got = NF.nonfinite(ref64), NF.nonfinite(got)
    assert torch.equal(bad_got, bad), (f"{what}: {int(bad_got.sum())} non-finite elements, the fp64 reference has {int(bad.sum())}; "
                                       f"{int((bad_got & ~bad).sum())} only here, {int((bad & ~bad_got).sum())} only there")
    if check is not None:
        zero = lambda t: torch.where(bad, torch.zeros((), dtype=t.dtype), t)
        check(zero(got), None if ref32 is None else zero(ref32), zero(ref64), what, **kw)


def _abs(got, ref32, ref64, what, K):
    err = float((got.double() - ref64).abs().max())
    assert err <= _bound(K, ref64), f"{what}: {err:.3e} > {_bound(K, ref64):.3e}"


def _exact(got, ref32, ref64, what):
    assert torch.equal(got.double(), ref64), what


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------
def _bn_forward(cuda, c, d):
    """osi_bn_train_stats + osi_bn_apply [+ the bitmask forms] -> dict of GPU tensors (NHWC activations, [C] vectors)."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    M, C = c.B * c.H * c.H, c.C
    yg = T.nhwc(d["y"]).to(cuda)
    ga, be, rm, rv = (d[k].to(cuda).contiguous() for k in ("gamma", "beta", "rm0", "rv0"))
    st = {k: _full((C,), cuda) for k in ("mean", "invstd", "scale", "shift")}
    wsb = max(L.osi_bn_workspace(M, C), L.osi_bn_backward_workspace(M, C))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=cuda)
    N.check(L.osi_bn_train_stats(N.ptr(yg), M, C, N.ptr(ga), N.ptr(be), 1e-5, 0.1, N.ptr(rm), N.ptr(rv), N.ptr(st["mean"]), N.ptr(st["invstd"]),
                                 N.ptr(st["scale"]), N.ptr(st["shift"]), N.ptr(ws), wsb, T.S()), "osi_bn_train_stats")
    rg = T.nhwc(d["resid"]).to(cuda) if c.res else None
    out = _full(yg.shape, cuda)
    N.check(L.osi_bn_apply(N.ptr(yg), N.ptr(rg), N.ptr(st["scale"]), N.ptr(st["shift"]), N.ptr(out), M, C, int(c.relu), T.S()), "osi_bn_apply")
    r = dict(st, out=out, running_mean=rm, running_var=rv, y=yg, gamma=ga, ws=ws, wsb=wsb)
    if c.relu:
        mask = torch.zeros(L.osi_bn_relu_mask_bytes(M, C), dtype=torch.uint8, device=cuda)
        r["out_mask"] = _full(yg.shape, cuda)
        N.check(L.osi_bn_apply_relu_mask(N.ptr(yg), N.ptr(rg), N.ptr(st["scale"]), N.ptr(st["shift"]), N.ptr(r["out_mask"]), N.ptr(mask), M, C, T.S()),
                "osi_bn_apply_relu_mask")
        r["mask"] = mask
        if c.res:       # the shortcut through its own (identity) BatchNorm, applied on the fly: fma(res, 1, 0) is exact
            one, zero = torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
            r["out_mask2"], m2 = _full(yg.shape, cuda), torch.zeros_like(mask)
            N.check(L.osi_bn_apply_relu_mask2(N.ptr(yg), N.ptr(st["scale"]), N.ptr(st["shift"]), N.ptr(rg), N.ptr(one), N.ptr(zero),
                                              N.ptr(r["out_mask2"]), N.ptr(m2), M, C, T.S()), "osi_bn_apply_relu_mask2")
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("case", [c for c in NF.BN_CASES if c.operand == "y"], ids=NF.bn_id)
def test_batchnorm_forward(cuda, case):
    """One NaN / +Inf element of y: channel c0 of out, mean, invstd, scale, shift and the running statistics is non-finite exactly as
    in F.batch_norm, every other channel within test_batchnorm's bounds; the bitmask forms write the same activation."""
    import osi_testlib as T
    d = NF.bn_inputs(case)
    r32, r64 = NF.bn_ref(case, d, F32), NF.bn_ref(case, d, F64)
    g = _bn_forward(cuda, case, d)
    for k in NF.BN_FWD_OUTPUTS:
        got = T.nchw(g[k]) if k == "out" else g[k]
        _same(got, r32[k], r64[k], f"{NF.bn_id(case)} {k}")
    for k in ("out_mask", "out_mask2"):
        if k in g:
            _same(T.nchw(g[k]), r32["out"], r64["out"], f"{NF.bn_id(case)} {k}")


@pytest.mark.parametrize("case", [c for c in NF.BN_CASES if c.operand == "dout"], ids=NF.bn_id)
def test_batchnorm_backward(cuda, case):
    """Clean forward state, one NaN / +Inf element of dout. Gate open: dgamma, dbeta and dy of that channel are non-finite as in torch.
    Gate closed: everything finite and within test_batchnorm's bounds (a select takes the element out, not a multiply)."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    d = NF.bn_inputs(case)
    r32, r64 = NF.bn_ref(case, d, F32), NF.bn_ref(case, d, F64)
    g = _bn_forward(cuda, case, d)
    assert bool(torch.isfinite(g["out"]).all())
    M, C = case.B * case.H * case.H, case.C
    dog = T.nhwc(d["dout"]).to(cuda)
    forms = [("osi_bn_backward", N.ptr(g["out"]) if case.relu else None)] + ([("osi_bn_backward_relu_mask", N.ptr(g["mask"]))] if case.relu else [])
    for name, gate in forms:
        dy, gm, dg, db = _full(dog.shape, cuda), _full(dog.shape, cuda), _full((C,), cuda), _full((C,), cuda)
        N.check(getattr(L, name)(N.ptr(dog), gate, N.ptr(g["y"]), N.ptr(g["mean"]), N.ptr(g["invstd"]), N.ptr(g["gamma"]), N.ptr(dy), N.ptr(gm),
                                 N.ptr(dg), N.ptr(db), M, C, N.ptr(g["ws"]), g["wsb"], T.S()), name)
        torch.cuda.synchronize()
        what = f"{NF.bn_id(case)} {name}"
        _same(T.nchw(dy), r32["dy"], r64["dy"], what + " dy", slack=8.0, floor=5e-6)
        _same(dg, r32["dgamma"], r64["dgamma"], what + " dgamma", slack=8.0, floor=5e-6)
        _same(db, r32["dbeta"], r64["dbeta"], what + " dbeta", slack=8.0, floor=5e-6)
        _same(T.nchw(gm), None, r64["gm"], what + " masked upstream gradient", check=_exact)
        if case.expect == "none":
            assert all(bool(torch.isfinite(t).all()) for t in (dy, gm, dg, db)), what


# ---- convolution epilogue statistics + osi_bn_finalize_stats ---------------------------------------------------------------------
@pytest.mark.parametrize("case", NF.BNSTATS_CASES, ids=lambda c: f"H{c.H}")
def test_conv_epilogue_statistics(cuda, case):
    """One NaN input pixel of a 1x1 convolution: every output channel's statistics are NaN in every tile and every finalisation form
    (rows, wide, two-level; forced by the knobs as in _conv_bnstats_case)."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    c = case
    d = NF.bnstats_inputs(c)
    r64 = NF.bnstats_ref(c, d, F64)
    xg, wg = T.nhwc(d["x"]).to(cuda), T.krsc(d["w"]).to(cuda)
    desc = N.ConvDesc.make(c.B, c.H, c.H, c.Cin, c.Cout, c.k, c.stride, 0)
    M = c.B * desc.Ho * desc.Wo
    ga, be = torch.ones(c.Cout, device=cuda), torch.zeros(c.Cout, device=cuda)
    nb = L.osi_conv_fwd_bnstats_workspace(ctypes.byref(desc))
    y64 = torch.nn.functional.conv2d(d["x"].double(), d["w"].double(), None, c.stride, 0)
    forms_seen = set()
    for tile in NF.BNSTATS_TILES:
        ps = _full((nb // 4,), cuda)
        y = _full((c.B, desc.Ho, desc.Wo, c.Cout), cuda)
        P, rows = ctypes.c_int(), ctypes.c_int()
        N.check(L.osi_conv_fwd_bnstats(ctypes.byref(desc), N.ptr(xg), N.ptr(wg), N.ptr(y), tile, N.ptr(ps), nb, ctypes.byref(P), ctypes.byref(rows), T.S()),
                "osi_conv_fwd_bnstats")
        _same(T.nchw(y), None, y64, f"tile {tile} conv output", check=None)
        for single_p, wide_p in NF.BNSTATS_FORMS:
            out = {k: _full((c.Cout,), cuda) for k in ("mean", "invstd", "scale", "shift")}
            out["running_mean"], out["running_var"] = torch.zeros(c.Cout, device=cuda), torch.ones(c.Cout, device=cuda)
            with T.pinned_knobs(bn_single_p=single_p, bn_wide_p=wide_p):
                N.check(L.osi_bn_finalize_stats(N.ptr(ps), nb, P.value, rows.value, M, c.Cout, N.ptr(ga), N.ptr(be), 1e-5, 0.1,
                                                N.ptr(out["running_mean"]), N.ptr(out["running_var"]), N.ptr(out["mean"]), N.ptr(out["invstd"]),
                                                N.ptr(out["scale"]), N.ptr(out["shift"]), T.S()), "osi_bn_finalize_stats")
                torch.cuda.synchronize()
            forms_seen.add("rows" if P.value <= single_p else "wide" if P.value <= wide_p else "two-level")
            for k, v in out.items():
                _same(v, None, r64[k], f"tile {tile} single_p {single_p} wide_p {wide_p} ({P.value} partials) {k}", check=None)
    assert forms_seen == {"rows", "wide", "two-level"}


# ---- convolutions ----------------------------------------------------------------------------------------------------------------
def _conv_abi(cuda, c, d, op, tile=0, accumulate=False):
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    B, Cin, H, W = d["x"].shape
    Cout, k, stride, pad = d["w"].shape[0], d["k"], d["stride"], d["pad"]
    desc = N.ConvDesc.make(B, H, W, Cin, Cout, k, stride, pad)
    xg, wg, dyg = T.nhwc(d["x"]).to(cuda), T.krsc(d["w"]).to(cuda), T.nhwc(d["dy"]).to(cuda)
    if op == "fwd":
        y = _full((B, desc.Ho, desc.Wo, Cout), cuda)
        N.check(L.osi_conv_fwd(ctypes.byref(desc), N.ptr(xg), N.ptr(wg), N.ptr(y), tile, T.S()), "osi_conv_fwd")
        return T.nchw(y)
    if op == "dgrad":
        dx = d["base"].to(cuda).clone() if accumulate else _full((B, H, W, Cin), cuda)
        N.check(L.osi_conv_dgrad(ctypes.byref(desc), N.ptr(dyg), N.ptr(wg), N.ptr(dx), int(accumulate), tile, T.S()), "osi_conv_dgrad")
        return T.nchw(dx)
    nbytes = L.osi_conv_wgrad_workspace(ctypes.byref(desc))
    ws = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=cuda)
    dw = _full((Cout, k, k, Cin), cuda)
    N.check(L.osi_conv_wgrad(ctypes.byref(desc), N.ptr(dyg), N.ptr(xg), N.ptr(dw), N.ptr(ws), nbytes, T.S()), "osi_conv_wgrad")
    return T.oihw(dw)


_FL = lambda K: 2e-6 + 6e-8 * K ** 0.5          # the floor of test_conv_fwd_dgrad_wgrad


@pytest.mark.parametrize("case", NF.CONV_CASES, ids=NF.conv_id)
def test_convolutions(cuda, case):
    """osi_conv_fwd / osi_conv_dgrad (also accumulate = 1) / osi_conv_wgrad with the tiles and bounds of test_conv_fwd_dgrad_wgrad."""
    c = case
    d = NF.conv_inputs(c)
    r32, r64 = NF.conv_ref(c, d, F32), NF.conv_ref(c, d, F64)
    what = NF.conv_id(c)
    if c.op == "fwd":
        for tile in [0, 4] + ([1, 3] if c.Cout % 128 == 0 else []) + [2]:
            _same(_conv_abi(cuda, c, d, "fwd", tile), r32["y"], r64["y"], f"{what} tile {tile}", floor=_FL(c.Cin * c.k * c.k))
    elif c.op == "dgrad":
        for tile in [0, 4] + ([1, 3] if c.Cin % 128 == 0 else []) + [2]:
            _same(_conv_abi(cuda, c, d, "dgrad", tile), r32["dx"], r64["dx"], f"{what} tile {tile}", floor=_FL(c.Cout * c.k * c.k))
        _same(_conv_abi(cuda, c, d, "dgrad", 0, True), r32["dx_acc"], r64["dx_acc"], f"{what} accumulate", floor=_FL(c.Cout * c.k * c.k))
    else:
        _same(_conv_abi(cuda, c, d, "wgrad"), r32["dw"], r64["dw"], what, floor=_FL(c.B * d["dy"].shape[2] * d["dy"].shape[3]))


def test_conv_large_m_splitk(cuda):
    """test_conv_large_m_splitk's form (deep split-K, ragged last split): one NaN in dy reaches exactly the filters of that output
    channel through every split."""
    c = NF.SPLITK_CASE
    d = NF.conv_inputs(c)
    r32, r64 = NF.conv_ref(c, d, F32), NF.conv_ref(c, d, F64)
    dw = _conv_abi(cuda, c, d, "wgrad")
    _same(dw, r32["dw"], r64["dw"], "wgrad split-K", slack=6.0)
    bad = NF.nonfinite(dw.cpu())
    assert bool(bad[NF.CONV_K0].all()) and int(bad.sum()) == bad[NF.CONV_K0].numel()


def _wino_abi(cuda, c, d):
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    desc = N.ConvDesc.make(c.B, c.H, c.W, c.Cin, c.Cout, 3, 1, 1)
    xg, wg, dyg = T.nhwc(d["x"]).to(cuda), T.krsc(d["w"]).to(cuda), T.nhwc(d["dy"]).to(cuda)
    if c.op == "wgrad":
        nb = L.osi_conv_wgrad_wino_workspace(ctypes.byref(desc))
        ws = torch.zeros(nb, dtype=torch.uint8, device=cuda)
        dw = _full((c.Cout, 3, 3, c.Cin), cuda)
        N.check(L.osi_conv_wgrad_wino(ctypes.byref(desc), N.ptr(dyg), N.ptr(xg), None, None, N.ptr(dw), N.ptr(ws), nb, T.S()), "osi_conv_wgrad_wino")
        return T.oihw(dw)
    wb = L.osi_conv_wino_workspace(ctypes.byref(desc))
    ws = torch.zeros(wb, dtype=torch.uint8, device=cuda)
    if c.op == "fwd":
        assert L.osi_conv_wino_eligible(ctypes.byref(desc), 0) == 1
        y = _full((c.B, c.H, c.W, c.Cout), cuda)
        N.check(L.osi_conv_fwd_wino(ctypes.byref(desc), N.ptr(xg), None, None, N.ptr(wg), N.ptr(y), N.ptr(ws), wb, None, 0, None, None, T.S()),
                "osi_conv_fwd_wino")
        return T.nchw(y)
    assert L.osi_conv_wino_eligible(ctypes.byref(desc), 1) == 1
    # the fused input gradient recomputes the producer's gate from y0 * scale0 + shift0: 1 * 1 + 1 > 0, open everywhere
    M = c.B * c.H * c.W
    y0, one, zero = torch.ones(M, c.Cin, device=cuda), torch.ones(c.Cin, device=cuda), torch.zeros(c.Cin, device=cuda)
    f = T.Fusion(None, y0.data_ptr(), zero.data_ptr(), one.data_ptr(), None, None, None, None, 0, one.data_ptr(), one.data_ptr())
    dx = _full((c.B, c.H, c.W, c.Cin), cuda)
    P = ctypes.c_int()
    N.check(L.osi_conv_dgrad_fused_wino(ctypes.byref(desc), N.ptr(dyg), N.ptr(wg), N.ptr(dx), ctypes.byref(f), N.ptr(ws), wb, ctypes.byref(P), T.S()),
            "osi_conv_dgrad_fused_wino")
    return T.nchw(dx)


# the forward form needs whole 16-tile statistics groups (osi_conv_wino_eligible): 5 images of 5 x 3 tiles have 75
_WINO = [c for c in NF.WINO_CASES if c.op != "fwd" or (c.B * ((c.H + 1) // 2) * ((c.W + 1) // 2)) % 16 == 0]


@pytest.mark.parametrize("case", _WINO, ids=NF.conv_id)
def test_winograd_forms(cuda, case):
    """osi_conv_fwd_wino, osi_conv_dgrad_fused_wino and osi_conv_wgrad_wino under the per-kernel bound of tests/test_wino_gpu.py. The
    transforms may turn Inf - Inf into NaN: the kind of non-finite value is not compared."""
    import osi_testlib as T
    c = case
    d = NF.conv_inputs(c, c.W)
    r64 = NF.conv_ref(c, d, F64)
    key, K = {"fwd": ("y", c.Cin * 9), "dgrad": ("dx", c.Cout * 9), "wgrad": ("dw", c.B * c.H * c.W)}[c.op]
    with T.pinned_knobs(wino_streamk=1):       # both directions cut stream-K, as tests/test_wino_gpu.py runs them
        _same(_wino_abi(cuda, c, d), None, r64[key], NF.conv_id(c), check=_abs, K=K)


# ---- fused-activation loaders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NF.ACT_CASES, ids=NF.act_id)
def test_fused_activation_loaders(cuda, case):
    """conv(relu(x * scale + shift) [+ res], w) with the activation recomputed in the operand loader: one NaN element of x, or a NaN
    shift (a whole NaN channel), reaches the outputs the materialised activation would reach (bounds of tests/test_fused_act_gpu.py
    and tests/test_wino_gpu.py: the direct kernels' per-kernel bound)."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    c = case
    d = NF.act_inputs(c)
    r64 = NF.act_ref(c, d, F64)
    desc = N.ConvDesc.make(c.B, c.H, c.H, c.Cin, c.Cout, c.k, c.stride, c.k // 2)
    x, sc, sh, w, dy = (d[k].to(cuda).contiguous() for k in ("x", "sc", "sh", "w", "dy"))
    what = NF.act_id(c)
    if c.entry in ("fwd_act", "fwd_rows", "fwd_act2"):
        res = d["res"].to(cuda) if c.entry == "fwd_act2" else None
        pb = L.osi_conv_fwd_bnstats_workspace(ctypes.byref(desc))
        with T.pinned_knobs(fwd_rows=2 if c.entry == "fwd_rows" else 1):
            for tile in ((0,) if c.entry == "fwd_rows" else (0, 5, 6) if c.Cout % 128 == 0 else (0, 5)):
                y, ps = _full((c.B, desc.Ho, desc.Wo, c.Cout), cuda), _full((pb // 4,), cuda)
                P, rows = ctypes.c_int(), ctypes.c_int()
                if res is None:
                    N.check(L.osi_conv_fwd_act(ctypes.byref(desc), N.ptr(x), N.ptr(sc), N.ptr(sh), N.ptr(w), N.ptr(y), tile, N.ptr(ps), pb,
                                               ctypes.byref(P), ctypes.byref(rows), T.S()), "osi_conv_fwd_act")
                else:
                    N.check(L.osi_conv_fwd_act2(ctypes.byref(desc), N.ptr(x), N.ptr(sc), N.ptr(sh), N.ptr(res), N.ptr(w), N.ptr(y), tile, N.ptr(ps), pb,
                                                ctypes.byref(P), ctypes.byref(rows), T.S()), "osi_conv_fwd_act2")
                _same(y, None, r64["y"], f"{what} tile {tile}", check=_abs, K=c.Cin * c.k * c.k)
    elif c.entry == "wgrad_act":
        nb = L.osi_conv_wgrad_workspace(ctypes.byref(desc))
        ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device=cuda)
        dw = _full((c.Cout, c.k, c.k, c.Cin), cuda)
        N.check(L.osi_conv_wgrad_act(ctypes.byref(desc), N.ptr(dy), N.ptr(x), N.ptr(sc), N.ptr(sh), N.ptr(dw), N.ptr(ws), nb, T.S()), "osi_conv_wgrad_act")
        _same(dw, None, r64["dw"], what, check=_abs, K=c.B * desc.Ho * desc.Wo)
    elif c.entry == "fwd_wino":
        wb = L.osi_conv_wino_workspace(ctypes.byref(desc))
        ws = torch.zeros(wb, dtype=torch.uint8, device=cuda)
        y = _full((c.B, c.H, c.H, c.Cout), cuda)
        N.check(L.osi_conv_fwd_wino(ctypes.byref(desc), N.ptr(x), N.ptr(sc), N.ptr(sh), N.ptr(w), N.ptr(y), N.ptr(ws), wb, None, 0, None, None, T.S()),
                "osi_conv_fwd_wino")
        _same(y, None, r64["y"], what, check=_abs, K=c.Cin * 9)
    else:
        nb = L.osi_conv_wgrad_wino_workspace(ctypes.byref(desc))
        ws = torch.zeros(nb, dtype=torch.uint8, device=cuda)
        dw = _full((c.Cout, 3, 3, c.Cin), cuda)
        N.check(L.osi_conv_wgrad_wino(ctypes.byref(desc), N.ptr(dy), N.ptr(x), N.ptr(sc), N.ptr(sh), N.ptr(dw), N.ptr(ws), nb, T.S()), "osi_conv_wgrad_wino")
        _same(dw, None, r64["dw"], what, check=_abs, K=c.B * c.H * c.H)


# ---- inference epilogues ---------------------------------------------------------------------------------------------------------
def _epi_bound(got, ref32, ref64, what, K, conv64, sc_max):
    """the bound of _epilogue_case (tests/test_eval_fused_gpu.py): the direct kernels' bound on the convolution, carried through the affine"""
    bound = _bound(K, conv64) * sc_max + 4e-7 * float(ref64.abs().max())
    err = float((got.double() - ref64).abs().max())
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def _epi_launch(cuda, c, d, wino):
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    desc = N.ConvDesc.make(c.B, c.H, c.H, c.Cin, c.Cout, c.k, 1, c.k // 2)
    M = c.B * c.H * c.H
    x, w, sc, sh = (d[k].to(cuda).contiguous() for k in ("x", "w", "sc", "sh"))
    res = d["res"].to(cuda) if c.shortcut else None
    out = _full((M, c.Cout), cuda)
    e = N.ConvEpilogue(sc.data_ptr(), sh.data_ptr(), None if res is None else res.data_ptr(), int(c.relu))
    if wino:
        ub, sb = L.osi_conv_wino_weights_bytes(ctypes.byref(desc)), L.osi_conv_wino_slab_bytes()
        u, slab = torch.zeros(ub, dtype=torch.uint8, device=cuda), torch.zeros(sb, dtype=torch.uint8, device=cuda)
        N.check(L.osi_conv_wino_transform_weights(ctypes.byref(desc), N.ptr(w), 0, N.ptr(u), ub, T.S()))
        N.check(L.osi_conv_fwd_wino_epilogue_pre(ctypes.byref(desc), N.ptr(x), N.ptr(u), N.ptr(out), ctypes.byref(e), N.ptr(slab), sb, T.S()),
                "osi_conv_fwd_wino_epilogue_pre")
    else:
        N.check(L.osi_conv_fwd_epilogue(ctypes.byref(desc), N.ptr(x), N.ptr(w), N.ptr(out), ctypes.byref(e), None, 0, T.S()), "osi_conv_fwd_epilogue")
    torch.cuda.synchronize()
    return out.view(c.B, c.H, c.H, c.Cout).cpu()


def _epilogue_case(cuda, c, wino):
    clean, bad = NF.epi_inputs(c)
    r64 = NF.epi_ref(c, bad, F64)["out"]
    conv64 = NF.epi_ref(c._replace(relu=False, shortcut=False), dict(clean, sc=torch.ones(c.Cout), sh=torch.zeros(c.Cout)), F64)["out"]
    got0, got = _epi_launch(cuda, c, clean, wino), _epi_launch(cuda, c, bad, wino)
    _same(got, None, r64, NF.epi_id(c), check=_epi_bound, K=c.Cin * c.k * c.k, conv64=conv64, sc_max=float(clean["sc"].max()))
    assert bool(torch.isfinite(got0).all())
    untouched = ~NF.nonfinite(r64)
    if c.operand == "x":       # the other images do not see the pixel at all
        untouched = torch.zeros_like(untouched); untouched[[i for i in range(c.B) if i != NF.EPI_IMAGE]] = True
    assert torch.equal(got[untouched], got0[untouched]), "everything the poison cannot reach is bit-identical to the clean launch"


@pytest.mark.parametrize("case", NF.EPI_CASES, ids=NF.epi_id)
def test_conv_epilogue(cuda, case):
    """osi_conv_fwd_epilogue (relu x shortcut): a NaN pixel of image 2 contaminates only its receptive field in image 2, a NaN shortcut
    element that one output, scale[n] = NaN channel n; everything else is bit-identical to the clean launch."""
    _epilogue_case(cuda, case, False)


@pytest.mark.parametrize("case", NF.EPI_WINO_CASES, ids=NF.epi_id)
def test_winograd_epilogue(cuda, case):
    _epilogue_case(cuda, case, True)


# ---- pools -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NF.POOL_CASES, ids=NF.pool_id)
def test_max_pools(cuda, case):
    """osi_maxpool3x3s2_fwd / osi_bn_relu_maxpool_fwd + osi_maxpool3x3s2_bwd: a NaN makes every window holding it NaN and the index byte
    (low 7 bits) names a NaN element; +Inf wins its windows; -Inf behaves as in torch; the backward scatters to the element the index
    names. Finite outputs: exactly torch's (unfused), the fp32 fma of k_bn_apply (fused) within test_batchnorm's bound."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    c = case
    d = NF.pool_inputs(c)
    r32, r64 = NF.pool_ref(c, d, F32), NF.pool_ref(c, d, F64)
    Ho, Wo = r64["y"].shape[2:]
    xg = T.nhwc(d["x"]).to(cuda)
    yg = _full((c.B, Ho, Wo, c.C), cuda)
    idx = torch.full((c.B, Ho, Wo, c.C), 0x7f, dtype=torch.uint8, device=cuda)
    if c.fused:
        sc, sh = d["sc"].to(cuda), d["sh"].to(cuda)
        N.check(L.osi_bn_relu_maxpool_fwd(N.ptr(xg), N.ptr(sc), N.ptr(sh), N.ptr(yg), N.ptr(idx), c.B, c.H, c.W, c.C, T.S()), "osi_bn_relu_maxpool_fwd")
        _same(T.nchw(yg), r32["y"], r64["y"], NF.pool_id(c))
    else:
        N.check(L.osi_maxpool3x3s2_fwd(N.ptr(xg), N.ptr(yg), N.ptr(idx), c.B, c.H, c.W, c.C, T.S()), "osi_maxpool3x3s2_fwd")
        _same(T.nchw(yg), None, r64["y"], NF.pool_id(c), check=_exact)
    pos = (T.nchw(idx).cpu() & 0x7f).long()
    assert int(pos.max()) <= 8
    ho, wo = torch.arange(Ho).view(1, 1, -1, 1), torch.arange(Wo).view(1, 1, 1, -1)
    h, w = 2 * ho - 1 + pos // 3, 2 * wo - 1 + pos % 3
    assert bool(((h >= 0) & (h < c.H) & (w >= 0) & (w < c.W)).all()), "the index names an element inside the image"
    flat = h * c.W + w
    named = torch.gather(r64["act"].flatten(2), 2, flat.flatten(2)).view(r64["y"].shape)
    bad = NF.nonfinite(r64["y"])
    if c.value == "nan":
        assert bool(torch.isnan(named[bad]).all()), "the index of a NaN window names a NaN element"
    if c.value == "+inf":
        assert bool((T.nchw(yg).cpu()[bad] == NF.INF).all()) and bool((named[bad] == NF.INF).all())
    # backward: scatter of dy to the element the kernel's own index names (dy on a grid of 1/64: every sum is exact)
    dyg = T.nhwc(d["dy"]).to(cuda)
    dx = _full(xg.shape, cuda)
    if c.fused:      # bit 7 of the index byte = "maximum > 0", the stem's ReLU gate: not part of the position osi_maxpool3x3s2_bwd compares
        assert bool(((idx.cpu() & 0x80) != 0)[T.nhwc(r64["y"] > 1e-3)].all())
        idx = idx & 0x7f
    N.check(L.osi_maxpool3x3s2_bwd(N.ptr(dyg), N.ptr(idx), N.ptr(dx), c.B, c.H, c.W, c.C, T.S()), "osi_maxpool3x3s2_bwd")
    want = torch.zeros(c.B, c.C, c.H * c.W, dtype=torch.float64).scatter_add_(2, flat.flatten(2), d["dy"].double().flatten(2)).view(c.B, c.C, c.H, c.W)
    assert torch.equal(T.nchw(dx).cpu().double(), want), "max-pool backward scatters to the element the index names"
    if not c.fused:  # one poisoned element per window: no choice between NaNs, so torch's own gradient is the same
        assert torch.equal(want, r64["dx"])


@pytest.mark.parametrize("which", ["avgpool", "linear"])
def test_avgpool_and_linear(cuda, which):
    """osi_avgpool_* and osi_linear_*: one NaN in, the reference's rows out (sums propagate by themselves: pins what already holds)."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    L = N.lib()
    d = NF.avgpool_linear_inputs(which)
    r32, r64 = NF.avgpool_linear_ref(which, d, F32), NF.avgpool_linear_ref(which, d, F64)
    if which == "avgpool":
        B, HW, C = d["x"].shape
        xg, dyg = d["x"].to(cuda), d["dy"].to(cuda)
        y, dx = _full((B, C), cuda), _full((B, HW, C), cuda)
        N.check(L.osi_avgpool_fwd(N.ptr(xg), N.ptr(y), B, HW, C, T.S()))
        N.check(L.osi_avgpool_bwd(N.ptr(dyg), N.ptr(dx), B, HW, C, T.S()))
        _same(y, r32["y"], r64["y"], "avgpool fwd")
        _same(dx, r32["dx"], r64["dx"], "avgpool bwd")
        return
    x, w, b, dy = (d[k].to(cuda) for k in ("x", "w", "b", "dy"))
    B, K = x.shape
    O = w.shape[0]
    y, dx, dw, db = _full((B, O), cuda), _full((B, K), cuda), _full((O, K), cuda), _full((O,), cuda)
    N.check(L.osi_linear_fwd(N.ptr(x), N.ptr(w), N.ptr(b), N.ptr(y), B, K, O, T.S()))
    N.check(L.osi_linear_bwd(N.ptr(dy), N.ptr(x), N.ptr(w), N.ptr(dx), 0, N.ptr(dw), N.ptr(db), B, K, O, T.S()))
    for k, got in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        _same(got, r32[k], r64[k], f"linear {k}")


# ---- head ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NF.LOSS_CASES, ids=NF.loss_id)
def test_loss(cuda, case):
    """osi_loss_fwd_bwd, three modes: a NaN / +Inf logit in a counted row makes the loss and that row's dlogits non-finite as in torch, the
    other rows stay finite (bounds of tests/test_head_kernels_gpu.py); in a row torch ignores or refuses, whatever torch gives."""
    import head_cases as H
    from test_head_kernels_gpu import _launch_loss
    d = NF.loss_inputs(case)
    r64 = NF.loss_ref(case, d, F64)
    code, loss, dz, _ = _launch_loss(cuda, d["mode"], d["z"], d["y"], 1.0, d["cw"])
    assert code == 0
    what = NF.loss_id(case)
    assert bool(torch.isfinite(loss)) == bool(torch.isfinite(r64["loss"])), f"{what}: loss {float(loss)} vs {float(r64['loss'])}"
    if bool(torch.isfinite(r64["loss"])):
        _check_loss(loss, r64["loss"], what)
    n = H.normaliser(d["mode"], d["y"], NF.LOSS_C, d["cw"])
    zfin = torch.nan_to_num(d["z"], nan=0.0, posinf=0.0, neginf=0.0)
    _same(dz, None, r64["dz"], what, check=lambda g, _, r, w: _check_dlogits(g, r, zfin, n, w))
    bad = NF.nonfinite(dz)
    assert int(bad.sum()) == int(bad[d["row"]].sum())


@pytest.mark.parametrize("row", NF.OBJECTO_ROWS)
def test_objectosphere(cuda, row):
    """The objectosphere term: a NaN feature element makes the loss NaN and the whole dfeat row of that sample NaN (the norm is NaN, as
    in torch), whether the row is known (residual max(xi - |f|, 0)) or unknown (|f|); every other row and dlogits stay within the
    bounds of test_objectosphere_vs_fp64."""
    import head_cases as H
    from test_head_kernels_gpu import _check_dfeat, _launch_loss
    d = NF.objecto_inputs(row)
    r64 = NF.objecto_ref(d, F64)
    code, loss, dz, df = _launch_loss(cuda, H.ENTROPIC, d["z"], d["y"], 1.0, None, -1, d["f"], NF.OBJECTO_XI, NF.OBJECTO_ALPHA)
    assert code == 0 and bool(torch.isnan(loss)) and bool(torch.isnan(r64["loss"]))
    _same(dz, None, r64["dz"], f"objectosphere {row} dlogits", check=lambda g, _, r, w: _check_dlogits(g, r, d["z"], float(NF.LOSS_B), w))
    _same(df, None, r64["df"], f"objectosphere {row} dfeat", check=lambda g, _, r, w: _check_dfeat(g, r, w))
    assert bool(torch.isnan(df[d["row"]]).all())


def test_softmax(cuda):
    from openset_imagenet import _native as N
    import osi_testlib as T
    z = NF.softmax_inputs()
    zg, out = z.to(cuda), _full(z.shape, cuda)
    N.check(N.lib().osi_softmax(N.ptr(zg), N.ptr(out), z.shape[0], z.shape[1], T.S()))
    _same(out, None, torch.softmax(z.double(), 1), "softmax",
          check=lambda g, _, r, w: torch.testing.assert_close(g.double(), r, atol=1e-7, rtol=1e-5))      # the bound of test_softmax_vs_fp64


@pytest.mark.parametrize("form", ["scores", "logits"])
@pytest.mark.parametrize("row", ["known", "negative"])
def test_confidence(cuda, row, form):
    """osi_confidence_from_scores / osi_confidence_accumulate: a NaN in a known row makes acc4[0] NaN, in a row labelled unknown acc4[2]
    (the row maximum keeps the NaN, as torch.max in metrics.confidence); the other sum and both counts are the oracle's."""
    from openset_imagenet import _native as N
    import osi_testlib as T
    arg, y, offset, unk, _ = NF.conf_inputs(row, form)
    fn = N.lib().osi_confidence_from_scores if form == "scores" else N.lib().osi_confidence_accumulate
    ref = NF.conf_ref(arg, y, offset, unk, form, F64)
    ag, yg = arg.to(cuda).contiguous(), y.to(cuda)
    acc = torch.zeros(4, dtype=torch.float64, device=cuda)
    N.check(fn(N.ptr(ag), N.ptr(yg), arg.shape[0], arg.shape[1], float(offset), int(unk), 0, N.ptr(acc), T.S()))
    acc = acc.cpu()
    assert torch.equal(NF.nonfinite(acc), NF.nonfinite(ref)), f"{acc.tolist()} vs {ref.tolist()}"
    assert bool(torch.isnan(acc[0 if row == "known" else 2]))
    assert float(acc[1]) == float(ref[1]) > 0 and float(acc[3]) == float(ref[3]) > 0
    clean = 2 if row == "known" else 0          # the other mean: the bound of test_confidence_vs_oracle
    assert abs(float(acc[clean] / acc[clean + 1]) - float(ref[clean] / ref[clean + 1])) < 1e-6


# ---- whole network ---------------------------------------------------------------------------------------------------------------
def _model(cuda, sd):
    from openset_imagenet import ResNet50
    import osi_testlib as T
    model = ResNet50(T.NET_C, T.NET_C, False)
    model.load_state_dict(sd)
    return model.to(cuda)


@pytest.mark.parametrize("poison", NF.NET_POISONS)
def test_network_training_step_reports_nan(cuda, poison):
    """A NaN pixel in image 1, then a whole NaN filter in layer3.0.conv2.weight: the logits' and the BatchNorm buffers' non-finite
    masks equal the fp64 oracle's, the loss is NaN, and after backward() the gradient norm is not finite: a diverged run looks diverged."""
    from openset_imagenet import EntropicOpensetLoss
    from oracle import resnet50_oracle as R
    import osi_testlib as T
    sd, x, y, _ = NF.network_inputs(poison)
    model = _model(cuda, sd).train()
    logits, _ = model(x.to(cuda))
    j = EntropicOpensetLoss(T.NET_C, 1.0)(logits, y.to(cuda))
    torch.cuda.synchronize()
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    with torch.no_grad():
        lg64, _ = R.forward(sd64, x.double(), True)
    assert bool(NF.nonfinite(lg64).any())
    _same(logits, None, lg64, f"{poison} logits", check=None)
    assert bool(torch.isnan(j.detach())), f"loss {float(j)}"
    state = model.state_dict()
    checked = 0
    for k, v in sd64.items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            _same(state[k], None, v, f"{poison} {k}", check=None)
            checked += 1
    assert checked == 2 * 53
    j.backward()
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(model.flat_gradients().norm())), "the gradient norm of a diverged step must not be finite"


def test_network_eval_forward_keeps_the_other_images(cuda):
    """model.eval(), a NaN pixel in image 2: logits and features of rows 0, 1, 3 are bit-identical to the clean batch and row 2's
    non-finite mask equals the fp64 oracle's."""
    from oracle import resnet50_oracle as R
    sd, x, _, clean = NF.network_inputs("pixel", image=2)
    model = _model(cuda, sd).eval()
    with torch.no_grad():
        lg0, ft0 = (t.cpu().clone() for t in model(clean.to(cuda)))
        lg, ft = (t.cpu().clone() for t in model(x.to(cuda)))
        rl, rf = R.forward({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}, x.double(), False)
    rows = [0, 1, 3]
    assert bool(torch.isfinite(lg0).all()) and bool(torch.isfinite(ft0).all())
    assert torch.equal(lg[rows], lg0[rows]) and torch.equal(ft[rows], ft0[rows])
    _same(lg, None, rl, "eval logits", check=None)
    _same(ft, None, rf, "eval features", check=None)
    assert bool(NF.nonfinite(rl[2]).all())

"""GPU parity of the kernels that close the network (loss.hip, linear.hip, the pooling half of pool_layout.hip) at the shapes where
their fixed strides wrap: 16 waves over the rows, 64 lanes (or 256-float strides) over the columns, 7-pixel batches over HW.

Through the C ABI; every output buffer is NaN before the launch; every reference is plain torch on the CPU in float64
(tests/head_cases.py builds inputs and references, tests/test_head_reference_cpu.py shows the references right without a kernel).
Tolerances are the ones tests/test_kernels_gpu.py already uses:
  linear, pooling   _check_vs64 (slack 4, floor 2e-6); max pool forward bit for bit
  loss value        2e-6 * max(1, |J64|)
  dlogits           2e-7 + 1e-6 max|ref| + 2e-8 max|z|, both sides first multiplied by the batch normaliser (B, the count of used rows, or
                    the sum of weights), so that the absolute floor means at B = 15360 what it means at B = 16
  dfeat             1e-6 * max(1, max|ref|)
"""
import pytest
import torch
import torch.nn.functional as F

import head_cases as H

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _err(a, ref64):
    return float((a.double().cpu() - ref64).abs().max())


def _check_vs64(got, ref32, ref64, what, slack=4.0, floor=2e-6):
    """got must be as close to the fp64 truth as torch-CPU fp32 is (times slack), relative to the tensor's scale."""
    scale = float(ref64.abs().max()) + 1e-30
    e_got, e_ref = _err(got, ref64) / scale, _err(ref32, ref64) / scale
    assert e_got <= max(slack * e_ref, floor), f"{what}: rel err {e_got:.3e} vs torch-cpu-fp32 {e_ref:.3e}"


def _launch_loss(cuda, mode, z, y, w=1.0, cw=None, ignore_index=-1, feats=None, xi=0.0, alpha=0.0, want_grad=True):
    """(return code, loss, dlogits, dfeat) of one osi_loss_fwd_bwd launch, outputs poisoned with NaN."""
    from openset_imagenet import _native as N
    import osi_testlib as T
    zg, yg = z.to(cuda).contiguous(), y.to(cuda)
    loss = torch.full((), NAN, device=cuda)
    dz = torch.full_like(zg, NAN) if want_grad else None
    fg = feats.to(cuda).contiguous() if feats is not None else None
    df = torch.full_like(fg, NAN) if fg is not None else None
    cwg = cw.to(cuda).contiguous() if cw is not None else None
    code = N.lib().osi_loss_fwd_bwd(mode, N.ptr(zg), N.ptr(yg), z.shape[0], z.shape[1], float(w), int(ignore_index), N.ptr(cwg), N.ptr(fg),
                                    feats.shape[1] if feats is not None else 0, float(xi), float(alpha), N.ptr(loss), N.ptr(dz), N.ptr(df), T.S())
    torch.cuda.synchronize()
    return code, loss.cpu(), None if dz is None else dz.cpu(), None if df is None else df.cpu()


def _check_loss(loss, J64, what):
    err, tol = abs(float(loss) - float(J64)), 2e-6 * max(1.0, abs(float(J64)))
    print(f"{what}: loss {float(loss)!r} vs fp64 {float(J64)!r}: |err| {err:.3e} (bound {tol:.3e})")
    assert err <= tol, f"{what} loss {float(loss)} vs {float(J64)}"


def _check_dlogits(dz, ref_dz, z, n, what, scale=1.0):
    """The bound of test_losses_vs_reference_golden on n * dlogits (n = the batch normaliser); scale = a factor both sides carry."""
    assert not bool(torch.isnan(dz).any()), f"{what}: dlogits elements left unwritten"
    ref = ref_dz * n
    # expf(x) carries ~|x| ulp of relative error: scale the bound with the logit range
    tol = scale * (2e-7 + 1e-6 * float(ref.abs().max()) / scale + 2e-8 * float(z.abs().max()))
    err = float((dz.double() * n - ref).abs().max())
    print(f"{what}: n * dlogits max |err| {err:.3e} (bound {tol:.3e}, n = {n})")
    assert err <= tol, f"{what} dlogits: {err:.3e} > {tol:.3e}"


def _check_dfeat(df, ref_df, what, scale=1.0):
    """The bound of test_objectosphere_vs_oracle (row 0 is the f = 0 row, whose gradient is defined as 0)."""
    assert not bool(torch.isnan(df).any()), f"{what}: dfeat elements left unwritten"
    err, tol = float((df.double() - torch.nan_to_num(ref_df)).abs().max()), 1e-6 * max(scale, float(ref_df[1:].abs().max()))
    print(f"{what}: dfeat max |err| {err:.3e} (bound {tol:.3e})")
    assert err < tol, f"{what} dfeat: {err:.3e} >= {tol:.3e}"


# ---- loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.LOSS_SHAPES, ids=H.loss_id)
@pytest.mark.parametrize("mode", list(H.MODES))
def test_loss_vs_fp64(cuda, mode, case):
    """Loss and dlogits of every mode against torch.nn.CrossEntropyLoss in float64; the loss-only launch and a second launch give the
    same bits as the first."""
    m = H.MODES[mode]
    z, y, cw, _ = H.loss_case(m, case)
    B, C = z.shape
    J64, dz64 = H.loss_ref64(m, z, y, 1.0, cw, -1, masked=H.needs_mask(m, y, C))
    code, loss, dz, _ = _launch_loss(cuda, m, z, y, 1.0, cw)
    assert code == 0
    what = f"{mode} {H.loss_id(case)}"
    _check_loss(loss, J64, what)
    _check_dlogits(dz, dz64, z, H.normaliser(m, y, C, cw), what)
    ignored = H.row_kinds(m, y, C)[2]
    assert float(dz[ignored].abs().sum()) == 0, "rows without a loss term get an all-zero gradient row"
    _, loss_only, _, _ = _launch_loss(cuda, m, z, y, 1.0, cw, want_grad=False)
    assert torch.equal(loss, loss_only), "loss-only launch must give the same bits"
    _, loss2, dz2, _ = _launch_loss(cuda, m, z, y, 1.0, cw)
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2), "fixed summation order: two launches give equal bits"


@pytest.mark.parametrize("w", [0.5, 2.0])
def test_entropic_unknown_weight(cuda, w):
    z, y, _, _ = H.loss_case(H.ENTROPIC, (40, 65, 3.0, "mixed"))
    J64, dz64 = H.loss_ref64(H.ENTROPIC, z, y, w)
    code, loss, dz, _ = _launch_loss(cuda, H.ENTROPIC, z, y, w)
    assert code == 0
    _check_loss(loss, J64, f"entropic w={w}")
    _check_dlogits(dz, dz64, z, 40.0, f"entropic w={w}")


@pytest.mark.parametrize("mode", list(H.MODES))
def test_loss_batch_past_the_lds_limit_is_refused(cuda, mode):
    """B = 15 * 1024 + 1: lse[B] no longer fits. OSI_ERR_ARG, nothing launched, nothing written."""
    m = H.MODES[mode]
    B, C = H.LOSS_MAX_B + 1, 5
    z, y = torch.zeros(B, C), torch.zeros(B, dtype=torch.int64)
    code, loss, dz, _ = _launch_loss(cuda, m, z, y, 1.0, torch.ones(C) if m == H.GARBAGE else None)
    assert code == -1
    assert bool(torch.isnan(loss)) and bool(torch.isnan(dz).all()), "a refused call writes nothing"


_IGNORE = H.softmax_ignore_cases()


@pytest.mark.parametrize("case", _IGNORE, ids=[c[0] for c in _IGNORE])
def test_softmax_mode_ignore_index(cuda, case):
    """ignore_index -1, 0 and C - 1 against CrossEntropyLoss(ignore_index=...); every row ignored -> NaN like torch."""
    name, z, y, ii, _ = case
    J64, dz64 = H.loss_ref64(H.SOFTMAX, z, y, ignore_index=ii)
    code, loss, dz, _ = _launch_loss(cuda, H.SOFTMAX, z, y, ignore_index=ii)
    assert code == 0
    if bool(torch.isnan(J64)):
        assert bool(torch.isnan(loss)), f"{name}: all-ignored batch must give NaN like torch"
        return
    _check_loss(loss, J64, name)
    _check_dlogits(dz, dz64, z, H.normaliser(H.SOFTMAX, y, z.shape[1], ignore_index=ii), name)
    assert float(dz[y == ii].abs().sum()) == 0


_GARBAGE = H.garbage_cases()


@pytest.mark.parametrize("case", _GARBAGE, ids=[c[0] for c in _GARBAGE])
def test_garbage_mode_minus100_and_zero_weights(cuda, case):
    """A -100 label (what GarbageLoss hands the kernel as ignore_index, torch's default), weights with zeros, and a batch whose
    present classes all weigh 0 (NaN like torch), against CrossEntropyLoss(weight=...) on the whole batch."""
    name, z, y, cw, _ = case
    J64, dz64 = H.loss_ref64(H.GARBAGE, z, y, cw=cw)
    code, loss, dz, _ = _launch_loss(cuda, H.GARBAGE, z, y, cw=cw, ignore_index=-100)
    assert code == 0
    if bool(torch.isnan(J64)):
        assert bool(torch.isnan(loss)), f"{name}: a batch of total weight 0 must give NaN like torch"
        return
    _check_loss(loss, J64, name)
    _check_dlogits(dz, dz64, z, H.normaliser(H.GARBAGE, y, z.shape[1], cw), name)
    known = (y >= 0)
    weightless = ~known | (cw[y.clamp(min=0)] == 0)
    assert float(dz[weightless].abs().sum()) == 0, "a -100 row and a row of a weight-0 class get an all-zero gradient row"


@pytest.mark.parametrize("B,C", [(17, 65), (40, 130)])
@pytest.mark.parametrize("mode", list(H.MODES))
def test_label_past_the_last_class_has_no_term_and_no_gradient(cuda, mode, B, C):
    """dlogits is the gradient of the loss the same launch reports: a row with y >= C adds nothing to J and gets an all-zero
    dlogits row (entropic: the divisor stays B); the other rows equal the fp64 reference of the batch with that row's term removed."""
    m = H.MODES[mode]
    z, y, cw, _ = H.loss_case(m, (B, C, 3.0, "mixed"))
    y, rows = H.with_labels_past_the_end(y, C)
    J64, dz64 = H.loss_ref64(m, z, y, 1.0, cw, -1, masked=True)
    assert float(dz64[rows].abs().sum()) == 0
    code, loss, dz, _ = _launch_loss(cuda, m, z, y, 1.0, cw)
    assert code == 0
    assert float(dz[rows].abs().sum()) == 0 and not bool(torch.isnan(dz[rows]).any()), "y >= C: all-zero dlogits row"
    _check_loss(loss, J64, f"{mode} y>=C")
    _check_dlogits(dz, dz64, z, H.normaliser(m, y, C, cw), f"{mode} y>=C")


@pytest.mark.parametrize("B,C,Fd", H.OBJECTO_SHAPES, ids=[f"B{B}-C{C}-F{Fd}-{'FgtC' if Fd > C else 'FltC'}" for B, C, Fd in H.OBJECTO_SHAPES])
def test_objectosphere_vs_fp64(cuda, B, C, Fd):
    """F != C, more than one trip of the waves over the rows and of the lanes over F; a known row outside the sphere (dfeat row
    exactly 0), one inside, an unknown row and a zero row, in the first trip and in the last."""
    for xi, alpha, w in H.OBJECTO_PARAMS:
        z, y, f = H.objecto_case(B, C, Fd, xi, H.gen(21, B, C, Fd))
        J64, dz64, df64 = H.objecto_ref64(z, y, f, w, xi, alpha)
        code, loss, dz, df = _launch_loss(cuda, H.ENTROPIC, z, y, w, None, -1, f, xi, alpha)
        assert code == 0
        what = f"objectosphere B{B} C{C} F{Fd} xi{xi}"
        _check_loss(loss, J64, what)
        _check_dlogits(dz, dz64, z, float(B), what)
        _check_dfeat(df, df64, what)
        for base in ((0,) if B <= 16 else (0, B - 4)):
            assert float(df[base + H.ROW_OUTSIDE].abs().max()) == 0, "known row with |f| > xi: dfeat exactly 0"
            assert float(df[base + H.ROW_ZERO].abs().max()) == 0, "f = 0: dfeat defined as 0"
            assert float(df[base + H.ROW_INSIDE].abs().max()) > 0 and float(df[base + H.ROW_UNKNOWN].abs().max()) > 0
        _, loss_only, none, df_only = _launch_loss(cuda, H.ENTROPIC, z, y, w, None, -1, f, xi, alpha, want_grad=False)
        assert none is None and torch.equal(loss, loss_only) and torch.equal(df, df_only)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_python_losses_scaled_backward(cuda):
    """(2.5 * loss).backward() on plain leaf logits (and features) is 2.5 x the fp64 gradient, for every loss class."""
    from openset_imagenet.losses import EntropicOpensetLoss, GarbageLoss, ObjectosphereLoss, SoftmaxLoss
    B, C, Fd = 40, 65, 130
    for mode, make in (("entropic", lambda cw: EntropicOpensetLoss(C, 0.5)), ("softmax", lambda cw: SoftmaxLoss()), ("garbage", GarbageLoss)):
        m = H.MODES[mode]
        z, y, cw, _ = H.loss_case(m, (B, C, 3.0, "mixed"))
        if m == H.GARBAGE:
            y[y == -1] = -100       # what torch.nn.CrossEntropyLoss(weight=...) ignores, and what GarbageLoss hands the kernel
        w = 0.5 if m == H.ENTROPIC else 1.0
        J64, dz64 = H.loss_ref64(m, z, y, w, cw)
        zg = z.to(cuda).requires_grad_(True)
        j = make(cw)(zg, y.to(cuda))
        (2.5 * j).backward()
        _check_loss(j.detach().cpu(), J64, f"{mode} python")
        _check_dlogits(zg.grad.cpu(), 2.5 * dz64, z, H.normaliser(m, y, C, cw, -100 if m == H.GARBAGE else -1), f"{mode} python", scale=2.5)
    xi, alpha, w = H.OBJECTO_PARAMS[1]
    z, y, f = H.objecto_case(B, C, Fd, xi, H.gen(22))
    J64, dz64, df64 = H.objecto_ref64(z, y, f, w, xi, alpha)
    zg, fg = z.to(cuda).requires_grad_(True), f.to(cuda).requires_grad_(True)
    j = ObjectosphereLoss(C, w, xi, alpha)(zg, y.to(cuda), fg)
    (2.5 * j).backward()
    _check_loss(j.detach().cpu(), J64, "objectosphere python")
    _check_dlogits(zg.grad.cpu(), 2.5 * dz64, z, float(B), "objectosphere python", scale=2.5)
    _check_dfeat(fg.grad.cpu(), 2.5 * df64, "objectosphere python", scale=2.5)


@pytest.mark.parametrize("view", ["every_other_column", "transposed"])
def test_python_losses_noncontiguous_inputs(cuda, view):
    """Non-contiguous logits / features give the bits of their .contiguous() copies: loss and gradients."""
    from openset_imagenet.losses import ObjectosphereLoss
    B, C, Fd = 17, 65, 130
    xi, alpha, w = H.OBJECTO_PARAMS[1]
    g = H.gen(23)
    y = H.objecto_case(B, C, Fd, xi, g)[1].to(cuda)
    if view == "every_other_column":
        zb, fb = (torch.randn(B, 2 * n, generator=g).to(cuda).requires_grad_(True) for n in (C, Fd))
        zv, fv = zb[:, ::2], fb[:, ::2]
        back = lambda t: t[:, ::2]
    else:
        zb, fb = (torch.randn(n, B, generator=g).to(cuda).requires_grad_(True) for n in (C, Fd))
        zv, fv = zb.t(), fb.t()
        back = lambda t: t.t()
    assert not zv.is_contiguous() and not fv.is_contiguous()
    zc, fc = zv.detach().contiguous().requires_grad_(True), fv.detach().contiguous().requires_grad_(True)
    loss_fn = ObjectosphereLoss(C, w, xi, alpha)
    j_view, j_copy = loss_fn(zv, y, fv), loss_fn(zc, y, fc)
    assert torch.equal(j_view.detach(), j_copy.detach())
    j_view.backward()
    j_copy.backward()
    assert torch.equal(back(zb.grad), zc.grad) and torch.equal(back(fb.grad), fc.grad)
    if view == "every_other_column":
        assert float(zb.grad[:, 1::2].abs().max()) == 0 and float(fb.grad[:, 1::2].abs().max()) == 0


# ---- confidence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", H.CONF_SHAPES)
@pytest.mark.parametrize("form", ["scores", "logits"])
def test_confidence_vs_oracle(cuda, form, B, C):
    """Both kernels, C past the 64 lanes, every form of last_valid_class, both conventions of unknown_class, -2 rows counted on
    neither side; a second call on the same accumulator exactly doubles it."""
    from oracle import losses_oracle as LO
    from openset_imagenet import _native as N
    import osi_testlib as T
    fn = N.lib().osi_confidence_from_scores if form == "scores" else N.lib().osi_confidence_accumulate
    for unknown_class in (-1, C - 1):
        scores, y = H.conf_case(B, C, unknown_class, H.gen(31, B, C, unknown_class + 1))
        offset = 1.0 / C if unknown_class < 0 else 0.0
        arg = (scores if form == "scores" else torch.log(scores)).to(cuda).contiguous()     # softmax(log s) = s
        yg = y.to(cuda)
        for last in H.conf_last_valid(C):
            kn, kc, ng, nc = LO.confidence(scores.double(), y, offset, unknown_class, last)
            assert kc > 0 and nc > 0
            acc = torch.zeros(4, dtype=torch.float64, device=cuda)
            N.check(fn(N.ptr(arg), N.ptr(yg), B, C, float(offset), int(unknown_class), 0 if last is None else int(last), N.ptr(acc), T.S()))
            once = acc.cpu().clone()
            ks, kcount, ns, ncount = once.tolist()
            what = f"{form} B{B} C{C} unknown_class {unknown_class} last_valid_class {last}"
            print(f"{what}: known {ks / kcount - kn:+.3e}, unknown {ns / ncount - ng:+.3e}")
            assert (kcount, ncount) == (kc, nc), what
            assert abs(ks / kcount - kn) < 1e-6 and abs(ns / ncount - ng) < 1e-6, what
            N.check(fn(N.ptr(arg), N.ptr(yg), B, C, float(offset), int(unknown_class), 0 if last is None else int(last), N.ptr(acc), T.S()))
            assert torch.equal(acc.cpu(), 2 * once), f"{what}: the second call must add the same four values"


# ---- softmax ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C", H.SOFTMAX_SHAPES)
def test_softmax_vs_fp64(cuda, B, C):
    from openset_imagenet import _native as N
    import osi_testlib as T
    z = H.softmax_case(B, C, H.gen(41, B, C))
    zg = z.to(cuda)
    out = torch.full((B, C), NAN, device=cuda)
    N.check(N.lib().osi_softmax(N.ptr(zg), N.ptr(out), B, C, T.S()))
    out = out.cpu()
    assert not bool(torch.isnan(out).any())
    ref = torch.softmax(z.double(), 1)
    print(f"softmax B{B} C{C}: max |err| {float((out.double() - ref).abs().max()):.3e}, max |row sum - 1| {float((out.double().sum(1) - 1).abs().max()):.3e}")
    assert torch.allclose(out.double(), ref, atol=1e-7, rtol=1e-5)
    assert float((out.double().sum(1) - 1).abs().max()) <= 1e-6
    if B >= 3:
        assert float(out[1, ::3].abs().max()) == 0, "-inf logits have probability exactly 0"


# ---- linear ----------------------------------------------------------------------------------------------------------------------
def _linear_bwd(cuda, dy, x, w, dx, acc, dw, db):
    from openset_imagenet import _native as N
    import osi_testlib as T
    B, K = x.shape
    N.check(N.lib().osi_linear_bwd(N.ptr(dy), N.ptr(x), N.ptr(w), N.ptr(dx), acc, N.ptr(dw), N.ptr(db), B, K, w.shape[0], T.S()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,K,O", H.LINEAR_SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_linear_vs_fp64(cuda, B, K, O, bias):
    """K = 116 / 152 / 260 / 4: the f32x4 loop of the forward with a partial last stride; O = 1 and 9: a partial block of waves."""
    from openset_imagenet import _native as N
    import osi_testlib as T
    x, w, b, dy = H.linear_case(B, K, O, H.gen(51, B, K, O))
    r32, r64 = (H.linear_ref(x, w, b if bias else None, dy, dt) for dt in (torch.float32, torch.float64))
    xg, wg, bg, dyg = x.to(cuda), w.to(cuda), b.to(cuda), dy.to(cuda)
    y = torch.full((B, O), NAN, device=cuda)
    N.check(N.lib().osi_linear_fwd(N.ptr(xg), N.ptr(wg), N.ptr(bg) if bias else None, N.ptr(y), B, K, O, T.S()))
    _check_vs64(y, r32[0], r64[0], "linear fwd")
    dx, dw, db = (torch.full_like(t, NAN) for t in (xg, wg, bg))
    _linear_bwd(cuda, dyg, xg, wg, dx, 0, dw, db if bias else None)
    _check_vs64(dx, r32[1], r64[1], "linear dx")
    _check_vs64(dw, r32[2], r64[2], "linear dw")
    if bias:
        _check_vs64(db, r32[3], r64[3], "linear db")
    else:
        assert bool(torch.isnan(db).all())


@pytest.mark.parametrize("B,K,O", H.LINEAR_SHAPES)
def test_linear_dx_accumulate(cuda, B, K, O):
    """dx_accumulate = 1 (the objectosphere path of the head's backward) adds to what dx holds; dx_accumulate = 0 overwrites it."""
    g = H.gen(52, B, K, O)
    x, w, _, dy = H.linear_case(B, K, O, g)
    prefill = torch.randn(B, K, generator=g)
    r32, r64 = (H.linear_ref(x, w, None, dy, dt) for dt in (torch.float32, torch.float64))
    xg, wg, dyg = x.to(cuda), w.to(cuda), dy.to(cuda)
    dx = prefill.to(cuda).clone()
    _linear_bwd(cuda, dyg, xg, wg, dx, 1, None, None)
    _check_vs64(dx, prefill + r32[1], prefill.double() + r64[1], "linear dx accumulate")
    plain = torch.full((B, K), NAN, device=cuda)
    _linear_bwd(cuda, dyg, xg, wg, plain, 0, None, None)
    dx0 = prefill.to(cuda).clone()
    _linear_bwd(cuda, dyg, xg, wg, dx0, 0, None, None)
    _check_vs64(dx0, r32[1], r64[1], "linear dx over a prefill")
    assert torch.equal(dx0, plain), "dx_accumulate = 0 must not read what dx holds"


@pytest.mark.parametrize("absent", ["dx", "dw"])
def test_linear_null_outputs_leave_memory_alone(cuda, absent):
    """dx = NULL / dw = NULL (a frozen prefix): the outputs asked for are right, and the NaN-poisoned memory between them, where the
    absent output would lie, is untouched."""
    B, K, O = 9, 152, 152
    x, w, b, dy = H.linear_case(B, K, O, H.gen(53))
    r32, r64 = (H.linear_ref(x, w, b, dy, dt) for dt in (torch.float32, torch.float64))
    xg, wg, dyg = x.to(cuda), w.to(cuda), dy.to(cuda)
    arena = torch.full((B * K + O * K + O,), NAN, device=cuda)          # [dx | dw | db]
    dx, dw, db = arena[:B * K].view(B, K), arena[B * K:B * K + O * K].view(O, K), arena[B * K + O * K:]
    _linear_bwd(cuda, dyg, xg, wg, None if absent == "dx" else dx, 0, None if absent == "dw" else dw, db)
    _check_vs64(db, r32[3], r64[3], "linear db")
    if absent == "dx":
        assert bool(torch.isnan(dx).all()), "dx = NULL: nothing written"
        _check_vs64(dw, r32[2], r64[2], "linear dw")
    else:
        assert bool(torch.isnan(dw).all()), "dw = NULL: nothing written"
        _check_vs64(dx, r32[1], r64[1], "linear dx")


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,Hh,W", H.MAXPOOL_SHAPES)
@pytest.mark.parametrize("kind", H.MAXPOOL_INPUTS)
def test_maxpool_vs_torch(cuda, kind, B, C, Hh, W):
    """H != W, C = 4, one-pixel-high images; inputs with negative maxima (a padded pixel must never win: "negative" and "randn" fail
    a kernel that lets 0 stand for the padding) and with ties. The kernel takes the first in-image pixel of a window unconditionally,
    and every window of a 3x3 / 2 / 1 pool holds one, so the value it starts its maximum from is never observable by itself."""
    import osi_testlib as T
    from openset_imagenet import _native as N
    x, dy = H.maxpool_case(B, C, Hh, W, kind, H.gen(61, B, C, Hh, W, len(kind)))
    y64, dx64 = H.maxpool_ref(x, dy)
    Ho, Wo = y64.shape[2:]
    xg = T.nhwc(x).to(cuda)
    yg = torch.full((B, Ho, Wo, C), NAN, device=cuda)
    idx = torch.full((B * Ho * Wo * C,), 255, dtype=torch.uint8, device=cuda)
    N.check(N.lib().osi_maxpool3x3s2_fwd(N.ptr(xg), N.ptr(yg), N.ptr(idx), B, Hh, W, C, T.S()))
    assert torch.equal(T.nchw(yg).cpu(), F.max_pool2d(x, 3, 2, 1)), "maxpool forward, bit for bit"
    assert torch.equal(T.nchw(yg).cpu().double(), y64)
    assert int(idx.max()) <= 8
    dx = torch.full_like(xg, NAN)
    dyg = T.nhwc(dy).to(cuda)
    N.check(N.lib().osi_maxpool3x3s2_bwd(N.ptr(dyg), N.ptr(idx), N.ptr(dx), B, Hh, W, C, T.S()))
    assert not bool(torch.isnan(dx).any())
    assert torch.allclose(T.nchw(dx).cpu().double(), dx64, atol=1e-6), "maxpool backward (first-max tie rule)"


@pytest.mark.parametrize("B,HW,C", H.AVGPOOL_SHAPES)
def test_avgpool_vs_fp64(cuda, B, HW, C):
    """HW below 7 and no multiple of 7: the tail loop of the forward."""
    from openset_imagenet import _native as N
    import osi_testlib as T
    x, dy = H.avgpool_case(B, HW, C, H.gen(71, HW, C))
    y64, dx64 = H.avgpool_ref64(x, dy)
    xg, dyg = x.to(cuda), dy.to(cuda)
    yg = torch.full((B, C), NAN, device=cuda)
    N.check(N.lib().osi_avgpool_fwd(N.ptr(xg), N.ptr(yg), B, HW, C, T.S()))
    print(f"avgpool HW{HW} C{C}: fwd max |err| {_err(yg, y64):.3e}")
    assert torch.allclose(yg.cpu().double(), y64, atol=1e-6)
    dx = torch.full_like(xg, NAN)
    N.check(N.lib().osi_avgpool_bwd(N.ptr(dyg), N.ptr(dx), B, HW, C, T.S()))
    print(f"avgpool HW{HW} C{C}: bwd max |err| {_err(dx, dx64):.3e}")
    assert torch.allclose(dx.cpu().double(), dx64, atol=1e-7)

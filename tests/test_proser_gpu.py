"""GPU: PROSER (ABI 23). The in-place pairwise mix bit for bit against the fp32 emulation of tests/proser_oracle.py; the loss kernel and
the scores against the fp64 oracle; the mix inside the executor (read back through osi_resnet50_debug_unit_input) at three cuts, under
frozen and batch statistics; the one-shot rule and the state errors; two training steps of the PROSER module.
Shapes: the smallest that reach every path (one unit, one tile, several tiles with a ragged end, the layer3 input of the real step);
the executor cases are the project's smallest whole-network case (B = 4 at 64 x 64, C = 10, tests/test_frozen_bn_gpu.py::_case)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import proser_oracle as P
from openset_imagenet import _native as N

pytestmark = pytest.mark.gpu

GUARD = 64             # floats of sentinel before and after a buffer
SENTINEL = -7.25
EPS32 = float(np.finfo(np.float32).eps)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _guarded(x_host, cuda):
    """(whole buffer, the [B, L] view in its middle) on the device, sentinels on both sides."""
    B, L = x_host.shape
    buf = torch.full((GUARD + B * L + GUARD,), SENTINEL, device=cuda)
    x = buf[GUARD:GUARD + B * L].view(B, L)
    x.copy_(torch.from_numpy(x_host))
    return buf, x


def _guards_ok(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _mix(x_host, partner, weight, cuda):
    buf, x = _guarded(x_host, cuda)
    N.ops().mix_rows_pairs(x, torch.from_numpy(np.asarray(partner, dtype=np.int32)).to(cuda),
                           torch.from_numpy(np.asarray(weight, dtype=np.float32)).to(cuda))
    torch.cuda.synchronize()
    assert _guards_ok(buf), "the mix wrote outside its buffer"
    return x.cpu().numpy()


# ---- the mix kernel --------------------------------------------------------------------------------------------------------------------
MIX_SHAPES = {(2, 4): [1, 0], (6, 4): [3, 5, 4, 0, 2, 1], (5, 4100): [2, 3, 0, 1, 4], (8, 28 * 28 * 512): [7, 2, 1, 5, 6, 3, 4, 0]}


@pytest.mark.parametrize("kind", ["zero", "one", "quarter", "random"])
@pytest.mark.parametrize("shape", list(MIX_SHAPES))
def test_mix_bit_for_bit(cuda, shape, kind):
    B, L = shape
    partner = np.array(MIX_SHAPES[shape], dtype=np.int32)
    assert P.is_involution(partner)
    gen = np.random.default_rng(B * 1000 + L % 997)
    x = gen.standard_normal((B, L)).astype(np.float32)
    w = {"zero": np.zeros(B), "one": np.ones(B), "quarter": np.full(B, 0.25), "random": gen.random(B)}[kind].astype(np.float32)
    got = _mix(x, partner, w, cuda)
    want = P.mix_rows_pairs_f32(x, partner, w)
    assert np.array_equal(_bits(got), _bits(want))
    if kind == "zero":
        assert np.array_equal(_bits(got), _bits(x[partner])), "weight 0 is an exact swap"
    if kind == "one":
        assert np.array_equal(_bits(got), _bits(x)), "weight 1 is the identity"


def test_mix_rows_without_a_partner_keep_every_bit(cuda):
    """partner -1, B and the row itself: not read, not written (a NaN payload survives); a table that is no involution and holds wild
    values stays inside the buffer."""
    gen = np.random.default_rng(9)
    x = gen.standard_normal((6, 4100)).astype(np.float32)
    _bits(x)[2, :] = 0x7FC12345                       # quiet NaNs with a payload
    _bits(x)[3, ::2] = 0x7F800001 | 0x00400000
    partner = np.array([1, 0, -1, 6, 5, 4], dtype=np.int32)
    w = gen.random(6).astype(np.float32)
    got = _mix(x, partner, w, cuda)
    assert np.array_equal(_bits(got)[2:4], _bits(x)[2:4])
    want = P.mix_rows_pairs_f32(x, partner, w)
    assert np.array_equal(_bits(got)[[0, 1, 4, 5]], _bits(want)[[0, 1, 4, 5]])
    wild = np.array([3, 3, 3, 7, -5, 100, 2 ** 31 - 1, -2 ** 31], dtype=np.int64).astype(np.int32)
    y = gen.standard_normal((8, 260)).astype(np.float32)
    got = _mix(y, wild, gen.random(8).astype(np.float32), cuda)             # (the guard bands are checked inside)
    assert np.array_equal(_bits(got)[4:7], _bits(y)[4:7])


def test_mix_nan_and_inf_reach_only_their_pair(cuda):
    gen = np.random.default_rng(10)
    x = gen.standard_normal((4, 4100)).astype(np.float32)
    x[0, ::3] = np.nan
    x[0, 1::3] = np.inf
    x[0, 2::3] = -np.inf
    partner = np.array([1, 0, 3, 2], dtype=np.int32)
    w = np.array([0.5, 0.0, 0.3, 0.7], dtype=np.float32)
    got = _mix(x, partner, w, cuda)
    want = P.mix_rows_pairs_f32(x, partner, w)
    assert np.array_equal(_bits(got)[2:], _bits(want)[2:]) and np.isfinite(got[2:]).all()
    assert np.array_equal(np.isnan(got[:2]), np.isnan(want[:2]))
    ok = ~np.isnan(want[:2])
    assert np.array_equal(_bits(got[:2][ok]), _bits(want[:2][ok]))
    assert np.isnan(got[1]).any() and np.isnan(got[0]).any()


def test_mix_op_refuses_bad_tensors(cuda):
    x = torch.zeros(4, 8, device=cuda)
    p, w = torch.zeros(4, dtype=torch.int32, device=cuda), torch.ones(4, device=cuda)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        N.ops().mix_rows_pairs(torch.zeros(4, 6, device=cuda), p, w)
    with pytest.raises(RuntimeError, match="one entry per row"):
        N.ops().mix_rows_pairs(x, p[:3], w[:3])
    with pytest.raises(RuntimeError, match="dtype"):
        N.ops().mix_rows_pairs(x, p.long(), w)
    with pytest.raises(RuntimeError, match="aligned"):
        N.ops().mix_rows_pairs(torch.zeros(4 * 8 + 1, device=cuda)[1:].view(4, 8), p, w)


# ---- the loss kernel -------------------------------------------------------------------------------------------------------------------
LAMBDAS = (0.01, 1.0, 1.0)
LOSS_CASES = [(1, 0, 1, 1, 3.0), (2, 2, 1, 1, 3.0), (7, 4, 30, 5, 3.0), (130, 64, 151, 3, 3.0), (9, 4, 65, 1, 3.0),
              (7, 4, 30, 5, 80.0), (130, 64, 151, 3, 1e4)]


def _loss_inputs(B, n_mixed, C, D, scale):
    gen = np.random.default_rng(B * 7919 + C * 31 + D + int(scale))
    z = (gen.standard_normal((B, C)) * scale).astype(np.float32)
    d = (gen.standard_normal((B, D)) * scale).astype(np.float32)
    y = gen.integers(0, C, size=B).astype(np.int64)
    if B - n_mixed >= 4:
        y[-1], y[-2] = -1, C                     # clean rows without a term
    return z, d, y


def _loss_errors(got4, gdz, gdd, ref):
    """(loss error, gradient error) against the fp64 oracle: the four loss values relative to max(1, |value|); the gradient as the
    largest absolute error over [dlogits | ddummy] relative to the largest gradient entry."""
    r4, rdz, rdd = ref
    e_loss = float(np.max(np.abs(np.asarray(got4, dtype=np.float64) - r4) / np.maximum(1.0, np.abs(r4))))
    top = max(float(np.abs(rdz).max()), float(np.abs(rdd).max()), 1e-300)
    e_grad = max(float(np.abs(np.asarray(gdz, dtype=np.float64) - rdz).max()), float(np.abs(np.asarray(gdd, dtype=np.float64) - rdd).max())) / top
    return e_loss, e_grad


@functools.lru_cache(maxsize=None)
def _loss_reference(case):
    z, d, y = _loss_inputs(*case)
    return P.loss_and_grads(z, d, y, case[1], LAMBDAS)


@functools.lru_cache(maxsize=None)
def _loss_bars():
    """The bars are measured, not chosen: torch's fp32 CPU evaluation of the plainly written formula (cross_entropy over
    cat([logits, max dummy]), autograd for the gradients) against the fp64 oracle on the inputs of LOSS_CASES, the worst case of the
    list; the device may be 4 times as far (headroom over summation-order differences). Returns (loss bar, gradient bar)."""
    worst_l = worst_g = 0.0
    for case in LOSS_CASES:
        z, d, y = _loss_inputs(*case)
        zt, dt = torch.tensor(z, requires_grad=True), torch.tensor(d, requires_grad=True)
        J, terms = P.torch_loss(zt, dt, torch.tensor(y), case[1], LAMBDAS)
        J.backward()
        e_l, e_g = _loss_errors(terms.detach().numpy(), zt.grad.numpy(), dt.grad.numpy(), _loss_reference(case))
        print(f"torch fp32 CPU vs fp64, case {case}: loss {e_l:.3e} grad {e_g:.3e}")
        worst_l, worst_g = max(worst_l, e_l), max(worst_g, e_g)
    print(f"bars (4 x worst): loss {4 * worst_l:.3e} grad {4 * worst_g:.3e}")
    return 4 * worst_l, 4 * worst_g


def _run_loss(z, d, y, n_mixed, cuda, lambdas=LAMBDAS, need_grad=True):
    """The kernel through the op, every output inside guard bands of its own (the op allocates: the C ABI is called directly)."""
    B, C = z.shape
    D = d.shape[1]
    zt, dt, yt = torch.from_numpy(z).to(cuda), torch.from_numpy(d).to(cuda), torch.from_numpy(y).to(cuda)
    b4 = torch.full((GUARD + 4 + GUARD,), SENTINEL, device=cuda)
    bz = torch.full((GUARD + B * C + GUARD,), SENTINEL, device=cuda)
    bd = torch.full((GUARD + B * D + GUARD,), SENTINEL, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * GUARD)
    rc = N.lib().osi_proser_loss_fwd_bwd(N.ptr(zt), N.ptr(dt), N.ptr(yt), B, C, D, n_mixed, *lambdas, off(b4),
                                         off(bz) if need_grad else None, off(bd) if need_grad else None, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert _guards_ok(b4) and _guards_ok(bz) and _guards_ok(bd), "the loss kernel wrote outside its outputs"
    if not need_grad:
        assert bool((bz == SENTINEL).all()) and bool((bd == SENTINEL).all())
    return (b4[GUARD:GUARD + 4].cpu().numpy(), bz[GUARD:GUARD + B * C].view(B, C).cpu().numpy(), bd[GUARD:GUARD + B * D].view(B, D).cpu().numpy())


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "B{}_m{}_C{}_D{}_s{:g}".format(*c))
def test_loss_vs_fp64_oracle(cuda, case):
    bar_l, bar_g = _loss_bars()
    z, d, y = _loss_inputs(*case)
    got = _run_loss(z, d, y, case[1], cuda)
    e_l, e_g = _loss_errors(*got, _loss_reference(case))
    print(f"device vs fp64, case {case}: loss {e_l:.3e} (bar {bar_l:.3e}) grad {e_g:.3e} (bar {bar_g:.3e})")
    assert e_l <= bar_l and e_g <= bar_g
    # two runs give the same bits; the loss-only form gives the same loss
    again = _run_loss(z, d, y, case[1], cuda)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    only = _run_loss(z, d, y, case[1], cuda, need_grad=False)
    assert np.array_equal(_bits(only[0]), _bits(got[0]))
    # a row's gradients sum to zero within rounding. The row is coef * (s - onehot) [+ coef' * (s' - onehot)] with s = exp(e - max) / sum:
    # the ones cancel exactly against the entry they are subtracted from only up to that entry's rounding, so the error scales with
    # the row's coefficients (l0 / n1, or (l1 + l2) / n2), not with the gradient that is left: the C + 1 roundings of the softmax sum at
    # worst, a few ulp per entry for expf, the division and the exponent (sum of s * |e - max| * eps <= eps * log(C + 1)): (C + 8) * eps,
    # the bound of the scores
    _, dz, dd = got
    B, n1, C = case[0], case[1], case[2]
    n2 = int(((y[n1:] >= 0) & (y[n1:] < C)).sum())
    coef = np.array([LAMBDAS[0] / n1 if i < n1 else (LAMBDAS[1] + LAMBDAS[2]) / max(n2, 1) for i in range(B)])
    rows = dz.astype(np.float64).sum(axis=1) + dd.astype(np.float64).sum(axis=1)
    assert (np.abs(rows) <= EPS32 * (C + 8) * coef).all(), (rows, coef)
    # rows without a term: exact zeros; a ddummy row has one entry
    r4, rdz, rdd = _loss_reference(case)
    assert np.array_equal(dz == 0, rdz == 0) or case[4] > 50      # (saturated softmax entries underflow to zero at large magnitudes)
    assert ((dd != 0).sum(axis=1) <= 1).all() and np.array_equal((dd != 0).any(axis=1), (rdd != 0).any(axis=1))


def test_loss_ties_labels_and_empty_terms(cuda):
    z, d, y = _loss_inputs(9, 4, 12, 4, 3.0)
    d[:, 1] = d[:, 3] = 9.0                      # tied dummy maxima: the gradient lands on the first
    y[4:] = [2, -1, 12, 3, 0]                    # clean labels -1 and C among valid ones
    loss4, dz, dd = _run_loss(z, d, y, 4, cuda)
    ref = P.loss_and_grads(z, d, y, 4, LAMBDAS)
    bar_l, bar_g = _loss_bars()
    e_l, e_g = _loss_errors(loss4, dz, dd, ref)
    assert e_l <= bar_l and e_g <= bar_g
    counting = [0, 1, 2, 3, 4, 7, 8]
    assert (dd[counting, 1] != 0).all() and not dd[:, [0, 2, 3]].any()
    assert not dz[[5, 6]].any() and not dd[[5, 6]].any()
    # no counting clean row: the two clean terms and their gradients are exact zeros, whatever the rows hold
    y[4:] = -1
    z[5, 2] = np.nan
    loss4, dz, dd = _run_loss(z, d, y, 4, cuda)
    assert loss4[2] == 0 and loss4[3] == 0 and np.isfinite(loss4).all() and not dz[4:].any() and not dd[4:].any()
    assert np.array_equal(_bits(loss4[0:1]), _bits(np.float32(LAMBDAS[0]) * loss4[1:2]))
    # no mixed row either: everything is an exact zero
    y[:4] = 12                                   # (rows 0 .. 3 are clean rows now: no label inside [0, C) anywhere)
    loss4, dz, dd = _run_loss(z, d, y, 0, cuda)
    assert not loss4.any() and not dz.any() and not dd.any()


def test_loss_nan_propagates_like_torch(cuda):
    z, d, y = _loss_inputs(8, 4, 6, 3, 3.0)
    y[:] = [0, 1, 2, 3, 4, 5, 0, -1]
    for row, in_dummy in ((1, False), (5, False), (2, True), (6, True)):
        zz, dd_in = z.copy(), d.copy()
        if in_dummy:
            dd_in[row, 1] = np.nan
        else:
            zz[row, 3] = np.nan
        loss4, dz, dd = _run_loss(zz, dd_in, y, 4, cuda)
        assert np.isnan(loss4[0]), (row, in_dummy)
        assert np.isnan(dz[row]).all(), (row, in_dummy)
        others = [i for i in range(7) if i != row]
        assert np.isfinite(dz[others]).all() and np.isfinite(dd[others]).all()
        if in_dummy:                            # a NaN counts as the largest dummy logit: the gradient lands there, the rest stays zero
            assert np.isnan(dd[row, 1]) and dd[row, 0] == 0 and dd[row, 2] == 0
    zz = z.copy()
    zz[7, 0] = np.nan                            # a clean row without a term: not counted, exact zero rows
    loss4, dz, dd = _run_loss(zz, d, y, 4, cuda)
    assert np.isfinite(loss4).all() and not dz[7].any() and not dd[7].any()


def test_loss_autograd_function_and_linear_ops(cuda):
    """ProserLoss and the dummy classifier's linear ops through autograd against the oracle and torch's own linear."""
    from openset_imagenet.proser import ProserLoss, _LinearFn
    gen = torch.Generator().manual_seed(4)
    f = torch.randn(7, 12, generator=gen).to(cuda).requires_grad_()
    w = (torch.randn(5, 12, generator=gen) * 0.3).to(cuda).requires_grad_()
    b = torch.randn(5, generator=gen).to(cuda).requires_grad_()
    z = torch.randn(7, 9, generator=gen).to(cuda).requires_grad_()
    y = torch.tensor([0, 1, 2, 3, 4, -1, 8], device=cuda)
    dummy = _LinearFn.apply(f, w, b)
    ref_dummy = f.detach().double().cpu() @ w.detach().double().cpu().T + b.detach().double().cpu()
    assert torch.allclose(dummy.detach().double().cpu(), ref_dummy, rtol=0, atol=1e-5)
    j, terms = ProserLoss.apply(z, dummy, y, 4, LAMBDAS)
    (2.0 * j).backward()
    r4, rdz, rdd = P.loss_and_grads(z.detach().cpu().numpy(), ref_dummy.numpy(), y.cpu().numpy(), 4, LAMBDAS)
    assert abs(float(j.detach()) - r4[0]) <= 1e-5 and np.allclose(terms.cpu().numpy(), r4, atol=1e-5)
    assert np.allclose(z.grad.cpu().numpy(), 2 * rdz, atol=1e-6)
    g = torch.from_numpy(2 * rdd)
    assert torch.allclose(b.grad.double().cpu(), g.sum(0), atol=1e-6)
    assert torch.allclose(w.grad.double().cpu(), g.T @ f.detach().double().cpu(), atol=1e-5)
    assert torch.allclose(f.grad.double().cpu(), g @ w.detach().double().cpu(), atol=1e-5)


# ---- scores ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,D", [(1, 1, 1), (7, 30, 5), (130, 151, 3)])
def test_scores_vs_fp64(cuda, B, C, D):
    """Bar: an entry p = exp(e - max) / sum carries the rounding of its exponent (eps * |e - max|, and p * |e - max| <= 1 / e), two ulp
    of expf, the C + 1 roundings of the sum at worst and one of the division: (C + 8) * eps absolutely, p <= 1."""
    z, d, _ = _loss_inputs(B, 0, C, D, 3.0)
    zt, dt = torch.from_numpy(z).to(cuda), torch.from_numpy(d).to(cuda)
    got = N.ops().proser_scores(zt, dt, 0.75).cpu().numpy()
    ref = P.scores(z, d, 0.75)
    tol = (C + 8) * EPS32
    assert got.shape == (B, C + 1)
    assert np.abs(got - ref).max() <= tol
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= tol
    # the bias shifts the last column's logit and nothing else: with values on a grid where d + bias is exact, the bits agree
    dq = np.round(d * 8) / 8
    a = N.ops().proser_scores(zt, torch.from_numpy(dq.astype(np.float32)).to(cuda), 0.5).cpu().numpy()
    b = N.ops().proser_scores(zt, torch.from_numpy((dq + 0.5).astype(np.float32)).to(cuda), 0.0).cpu().numpy()
    assert np.array_equal(_bits(a), _bits(b))
    d[0, D - 1] = np.nan
    nan = N.ops().proser_scores(zt, torch.from_numpy(d).to(cuda), 0.0).cpu().numpy()
    assert np.isnan(nan[0]).all() and np.isfinite(nan[1:]).all()


def test_fit_bias_and_predict(cuda):
    from openset_imagenet import PROSER, ResNet50
    z, d, y = _loss_inputs(200, 0, 10, 5, 3.0)
    y[::7] = -1
    p = PROSER(ResNet50(10, 10, False), dummy_count=5)
    for rate in (0.95, 0.5, 1.0):
        assert p.fit_bias(z, d, y, known_rate=rate) is p
        assert float(p.bias) == P.fit_bias(z, d, y, rate)
    p.fit_bias(z, d, y)
    probs = p.predict(z, d)
    ref = P.scores(z, d, float(p.bias))
    assert probs.shape == (200, 11) and np.abs(probs.cpu().numpy() - ref).max() <= 18 * EPS32
    known = (y >= 0)
    kept = (z.max(axis=1) - d.max(axis=1))[known] >= float(p.bias)
    assert abs(kept.mean() - 0.95) <= 1.0 / known.sum() + 1e-12
    assert p.predict(z[:0], d[:0]).shape == (0, 11)
    with pytest.raises(ValueError, match="no known row"):
        p.fit_bias(z, d, np.full(200, -1))


# ---- the mix in the executor -----------------------------------------------------------------------------------------------------------
CUTS = ["layer1", "layer3", "layer4.2"]       # the producer is the stem's pool | projection block, side stream | identity block, residual reader
MODES = ["freeze_bn", "train"]
LOGIT_TOL, GRAD_TOL = 1e-4, 5e-4              # the suite's bars (tests/test_finetune_gpu.py)
PARTNER = [2, 3, 0, 1]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _net():
    from test_frozen_bn_gpu import _case, _model
    cuda = torch.device("cuda:0")
    sd, x, wl, wf = _case("signed")
    return dict(sd=sd, model=_model(sd, cuda), x=x.to(cuda), wl=wl.to(cuda), wf=wf.to(cuda))


def _unit_input(model, unit):
    net = model._last[0]
    L = N.lib()
    n = ctypes.c_size_t()
    assert L.osi_resnet50_debug_unit_input(net.h, None, unit, None, ctypes.byref(n), None) == 0
    out = torch.empty(n.value, device=model._flat_params.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.osi_resnet50_debug_unit_input(net.h, N.ptr(model._ws), unit, N.ptr(out), ctypes.byref(n), st) == 0
    return out.view(model._last[1].shape[0], -1)


def _step(cut, mode, mix=None, wl=None, wf=None):
    """Reload the state, one forward + loss + backward at `cut` in `mode`; mix = (partner list, weight list) or None."""
    c = _net()
    model, cuda = c["model"], c["x"].device
    model.load_state_dict(c["sd"])
    model.freeze_below(cut)
    model.train().freeze_bn(mode == "freeze_bn")
    model._flat_grads.fill_(float("nan"))
    for p in model.parameters():
        p.grad = None
    if mix is not None:
        model.next_forward(mix=(torch.tensor(mix[0], dtype=torch.int32, device=cuda), torch.tensor(mix[1], dtype=torch.float32, device=cuda)))
    logits, feats = model(c["x"])
    assert model._fw_request is None
    X = _unit_input(model, model._cut)
    wl, wf = c["wl"] if wl is None else wl, c["wf"] if wf is None else wf
    ((logits * wl).sum() + (feats * wf).sum()).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return dict(logits=logits.detach().clone(), feats=feats.detach().clone(), X=X, grads=grads, buffers=model._flat_buffers.clone(),
                nbt=model._nbt.clone())


@functools.lru_cache(maxsize=None)
def _plain(cut, mode):
    return _step(cut, mode)


def _same_bits(a, b, what):
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["feats"], b["feats"]), what
    assert a["grads"].keys() == b["grads"].keys() and len(a["grads"]) > 0
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), f"{what}: grad {k}"
    assert torch.equal(a["buffers"], b["buffers"]) and torch.equal(a["nbt"], b["nbt"]), what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cut", CUTS)
def test_executor_mixes_the_input_of_the_first_trainable_unit(cuda, cut, mode):
    plain = _plain(cut, mode)
    gen = np.random.default_rng(len(cut) + len(mode))
    w = gen.random(4).astype(np.float32)
    mixed = _step(cut, mode, mix=(PARTNER, w.tolist()))
    want = plain["X"].clone()
    N.ops().mix_rows_pairs(want, torch.tensor(PARTNER, dtype=torch.int32, device=cuda), torch.from_numpy(w).to(cuda))
    assert torch.equal(mixed["X"], want), "the suffix did not consume mix_rows_pairs(X)"
    assert np.array_equal(_bits(mixed["X"].cpu().numpy()), _bits(P.mix_rows_pairs_f32(plain["X"].cpu().numpy(), PARTNER, w)))
    assert not torch.equal(mixed["X"], plain["X"]) and not torch.equal(mixed["logits"], plain["logits"])
    assert bool(torch.isfinite(mixed["logits"]).all()) and all(bool(torch.isfinite(g).all()) for g in mixed["grads"].values())
    # one-shot: the next step without a request is the plain step, bit for bit
    _same_bits(_step(cut, mode), plain, "the step after a mixed step")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cut", CUTS)
def test_executor_mix_with_weights_one_is_the_plain_step(cuda, cut, mode):
    plain = _plain(cut, mode)
    one = _step(cut, mode, mix=(PARTNER, [1.0] * 4))
    assert torch.equal(one["X"], plain["X"])
    _same_bits(one, plain, "weights 1")


@pytest.mark.parametrize("cut", CUTS)
def test_executor_mix_with_weights_zero_swaps_the_rows(cuda, cut):
    """Under frozen statistics the rows are independent: with weights 0 row i IS row partner[i] from the cut on. Its logits are the
    partner's of the plain run, and with the head weights swapped the same way the loss is the same sum, so the suffix gradients are the
    plain run's (another summation order: the suite's bars)."""
    c = _net()
    plain = _plain(cut, "freeze_bn")
    perm = torch.tensor(PARTNER, device=cuda)
    swap = _step(cut, "freeze_bn", mix=(PARTNER, [0.0] * 4), wl=c["wl"][perm], wf=c["wf"][perm])
    assert torch.equal(swap["X"], plain["X"][perm])
    want = plain["logits"][perm]
    assert float((swap["logits"] - want).abs().max()) <= LOGIT_TOL * max(1.0, float(want.abs().max()))
    assert swap["grads"].keys() == plain["grads"].keys()
    for k, g in plain["grads"].items():
        assert _rel(swap["grads"][k], g) <= GRAD_TOL, k


def test_executor_mix_state_errors(cuda):
    c = _net()
    model, x = c["model"], c["x"]
    model.load_state_dict(c["sd"])
    model.train().freeze_bn(True)
    L = N.lib()
    partner = torch.tensor(PARTNER, dtype=torch.int32, device=cuda)
    weight = torch.full((4,), 0.5, device=cuda)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        # no cut and the cut "fc": refused on the host ...
        for cut in (None, "fc"):
            model.freeze_below(cut)
            with pytest.raises(ValueError, match="frozen_below"):
                model.next_forward(mix=(partner, weight))
            # ... and by the executor: OSI_ERR_STATE, nothing launched, the request stays until it is cleared
            model(x)
            net = model._last[0]
            torch.cuda.synchronize()
            assert L.osi_resnet50_set_mix(net.h, N.ptr(partner), N.ptr(weight)) == 0
            with pytest.raises(RuntimeError, match="osi_resnet50_forward"):
                model(x)
            with torch.no_grad():                  # an inference forward ignores the request and leaves it pending
                model(x)
            with pytest.raises(RuntimeError, match="osi_resnet50_forward"):
                model(x)
            assert L.osi_resnet50_set_mix(net.h, None, None) == 0
            model(x)
        model.freeze_below("layer3")
        # a wrong length is refused before the forward
        model.next_forward(mix=(partner[:3].contiguous(), weight[:3].contiguous()))
        with pytest.raises(ValueError, match="entries"):
            model(x)
        model.next_forward(mix=None)
        # a forward that does not run the prefix: an image that requires grad, a pending attack request
        model.next_forward(mix=(partner, weight))
        with pytest.raises(RuntimeError, match="does not run a frozen prefix"):
            model(x.clone().requires_grad_())
        with torch.no_grad():
            model(x)
        model.next_backward(fgsm=0.01)
        with pytest.raises(RuntimeError, match="does not run a frozen prefix"):
            model(x)
        model._bw_request = None
        with torch.no_grad():                      # a no-grad forward leaves the request pending
            model(x)
        assert model._fw_request is not None
        model.eval()
        model.freeze_bn(False)
        model(x)                                   # so does an inference forward with grad enabled
        assert model._fw_request is not None
        model.train().freeze_bn(True)
        logits, feats = model(x)                   # the forward that consumes it
        assert model._fw_request is None
        net = model._last[0]
        # dimage after a mix: OSI_ERR_STATE, as after every forward with an inference-form prefix; the plain backward still runs
        dl, dimg = torch.zeros_like(logits), torch.empty_like(x)
        assert L.osi_resnet50_backward_ex(net.h, N.ptr(model._flat_params), N.ptr(model._flat_grads), N.ptr(model._ws), N.ptr(dl), None,
                                          N.ptr(dimg), 1, 0, model._n_stages, st()) == -3
        (logits.sum() + feats.sum()).backward()
        torch.cuda.synchronize()
    finally:
        model._bw_request = None
        model._fw_request = None
        model.freeze_below(None)
        model.freeze_bn(False)


def test_two_training_steps_move_the_suffix_and_the_dummy_classifier_only(cuda):
    from openset_imagenet import PROSER, optim
    from test_finetune_cpu import unit_of_name
    from test_frozen_bn_gpu import _case, _model
    sd, x, _, _ = _case("signed")
    model = _model(sd, cuda)
    proser = PROSER(model, dummy_count=3, mix_at="layer3", generator=np.random.default_rng(1))
    assert proser.dummy_classifier.weight.device == model.flat_parameters().device
    cut = unit_of_name("resnet_base.layer3.0.conv1.weight")
    opt_model = optim.SGD(model, lr=1e-2, momentum=0.9)
    opt_dummy = torch.optim.SGD(proser.dummy_classifier.parameters(), lr=1e-2, momentum=0.9)
    labels = torch.tensor([3, 0, -1, 7], device=cuda)
    before = {k: v.detach().clone() for k, v in proser.state_dict().items() if isinstance(v, torch.Tensor)}
    xd = x.to(cuda)
    proser.train()
    for step in range(2):
        opt_model.zero_grad()
        opt_dummy.zero_grad()
        j = proser.training_step(xd, labels)
        j.backward()
        opt_model.step()
        opt_dummy.step()
        assert bool(torch.isfinite(j)) and bool(torch.isfinite(proser.terms).all()), step
        assert float(proser.terms[0]) == float(j.detach())
    torch.cuda.synchronize()
    after = proser.state_dict()
    for k, v in before.items():
        if k == "bias":
            assert torch.equal(after[k], v)
        elif k.startswith("dummy_classifier."):
            assert not torch.equal(after[k], v), f"{k}: the dummy classifier did not move"
        elif unit_of_name(k[len("model."):]) < cut:
            assert torch.equal(after[k], v), f"{k}: the frozen prefix changed"
        elif k.endswith("tracked"):
            assert int(after[k]) == int(v) + 2, k
        else:
            assert not torch.equal(after[k], v), f"{k}: the suffix did not move"
    # the scores of the fine-tuned module, end to end
    with torch.no_grad():
        model.eval()
        logits, dummy, _ = proser(xd)
    probs = proser.predict(logits, dummy)
    assert probs.shape == (4, 11) and bool(torch.isfinite(probs).all())

"""CPU: PROSER's host side (ABI 23). The symbols and the ctypes table; the fp64 oracle (tests/proser_oracle.py) against torch.autograd
of the plainly written formula; the published -1e9 form against the left-out-column form; draw_pairs; the bias index rule; every host
refusal; the no-GPU error."""
import ctypes

import numpy as np
import pytest
import torch

import proser_oracle as P
from openset_imagenet import _native as N

SYMBOLS = ["osi_mix_rows_pairs", "osi_proser_loss_fwd_bwd", "osi_proser_scores", "osi_resnet50_set_mix", "osi_resnet50_debug_unit_input"]


def _inputs(B, n_mixed, C, D, seed, scale=3.0):
    gen = np.random.default_rng(seed)
    z = (gen.standard_normal((B, C)) * scale).astype(np.float32)
    d = (gen.standard_normal((B, D)) * scale).astype(np.float32)
    y = gen.integers(0, C, size=B).astype(np.int64)
    return z, d, y


def test_symbols_are_exported_and_in_the_ctypes_table():
    lib = N.lib()
    assert lib.osi_abi_version() >= 23
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in N.declared_symbols(), s


def test_c_abi_refuses_bad_arguments_before_any_launch():
    lib = N.lib()
    assert lib.osi_mix_rows_pairs(None, 16, 16, 2, 4, None) == -1
    assert lib.osi_mix_rows_pairs(16, 16, 16, 2, 6, None) == -1          # L % 4 != 0
    assert lib.osi_mix_rows_pairs(16, 16, 16, 2, 0, None) == -1
    assert lib.osi_mix_rows_pairs(20, 16, 16, 2, 4, None) == -1          # x not 16-byte aligned
    assert lib.osi_mix_rows_pairs(16, 16, 16, 0, 4, None) == -1
    loss = lib.osi_proser_loss_fwd_bwd
    assert loss(16, 16, 16, 15361, 4, 2, 0, 1.0, 1.0, 1.0, 16, 16, 16, None) == -1      # B > 15360
    assert loss(16, 16, 16, 4, 4, 2, 5, 1.0, 1.0, 1.0, 16, 16, 16, None) == -1          # n_mixed > B
    assert loss(16, 16, 16, 4, 4, 2, -1, 1.0, 1.0, 1.0, 16, 16, 16, None) == -1
    assert loss(16, 16, 16, 4, 4, 0, 0, 1.0, 1.0, 1.0, 16, 16, 16, None) == -1          # D < 1
    assert loss(16, 16, 16, 4, 4, 2, 0, 1.0, 1.0, 1.0, 16, 16, None, None) == -1        # one gradient without the other
    assert loss(16, 16, 16, 4, 4, 2, 0, 1.0, 1.0, 1.0, None, 16, 16, None) == -1
    assert lib.osi_proser_scores(16, 16, 0.0, 4, 0, 2, 16, None) == -1
    assert lib.osi_proser_scores(16, None, 0.0, 4, 4, 2, 16, None) == -1
    h = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(h), 2, 64, 64, 10, 10, 0) == 0
    try:
        assert lib.osi_resnet50_set_mix(h, 16, None) == -1 and lib.osi_resnet50_set_mix(h, None, 16) == -1
        assert lib.osi_resnet50_set_mix(h, None, None) == 0
        n = ctypes.c_size_t()
        assert lib.osi_resnet50_debug_unit_input(h, None, 0, None, ctypes.byref(n), None) == -1
        assert lib.osi_resnet50_debug_unit_input(h, None, 17, None, ctypes.byref(n), None) == -1
        assert lib.osi_resnet50_debug_unit_input(h, None, 1, None, None, None) == -1
        sizes = []
        # 64 x 64 image: the pool leaves 16 x 16 x 64; units 1-3 layer1, 4-7 layer2, 8-13 layer3, 14-16 layer4; layerN.0 reads the layer below
        for unit in (1, 2, 4, 5, 8, 9, 14, 15, 16):
            assert lib.osi_resnet50_debug_unit_input(h, None, unit, None, ctypes.byref(n), None) == 0
            sizes.append(n.value)
        assert sizes == [2 * 16 * 16 * 64, 2 * 16 * 16 * 256, 2 * 16 * 16 * 256, 2 * 8 * 8 * 512, 2 * 8 * 8 * 512, 2 * 4 * 4 * 1024,
                         2 * 4 * 4 * 1024, 2 * 2 * 2 * 2048, 2 * 2 * 2 * 2048]
        assert lib.osi_resnet50_debug_unit_input(h, 16, 1, 16, ctypes.byref(n), None) == -3     # OSI_ERR_STATE: a copy before any forward
    finally:
        lib.osi_resnet50_destroy(h)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def test_fma_emulation_is_correctly_rounded():
    """Against exact rational arithmetic on values chosen to sit near rounding ties, and on random ones."""
    from fractions import Fraction
    gen = np.random.default_rng(3)
    a = gen.standard_normal(400).astype(np.float32)
    b = gen.standard_normal(400).astype(np.float32)
    c = (gen.standard_normal(400) * 10.0 ** gen.integers(-9, 3, 400)).astype(np.float32)
    a[:4] = np.float32(1 + 2 ** -23); b[:4] = np.float32(1 + 2 ** -23)
    c[:4] = np.array([2 ** -24, -2 ** -24, 2 ** -47, 2 ** 24], dtype=np.float32)
    got = P.fma_f32(a, b, c)
    for k in range(len(a)):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo = np.float32(float(exact))                       # a correctly rounded conversion of a Fraction goes through float() = fp64:
        cands = sorted({float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))})
        err = [abs(Fraction(v) - exact) for v in cands]     # so take the nearest of the fp32 neighbours exactly
        best = min(err)
        winners = [v for v, e in zip(cands, err) if e == best]
        if len(winners) > 1:                                # an exact tie: the even mantissa
            winners = [v for v in winners if (np.float32(v).view(np.int32) & 1) == 0]
        assert float(got[k]) == winners[0], (k, a[k], b[k], c[k])


def test_mix_emulation_identity_swap_and_fp64():
    gen = np.random.default_rng(5)
    x = gen.standard_normal((6, 8)).astype(np.float32)
    partner = np.array([3, 2, 1, 0, 4, 5], dtype=np.int32)
    assert P.is_involution(partner) and not P.is_involution(np.array([1, 2, 0]))
    ones = P.mix_rows_pairs_f32(x, partner, np.ones(6, dtype=np.float32))
    assert np.array_equal(ones, x)
    swap = P.mix_rows_pairs_f32(x, partner, np.zeros(6, dtype=np.float32))
    assert np.array_equal(swap, x[partner])
    w = gen.random(6).astype(np.float32)
    got = P.mix_rows_pairs_f32(x, partner, w)
    ref = P.mix_rows_pairs_f64(x, partner, w)
    assert np.abs(got - ref).max() <= 2 * np.finfo(np.float32).eps * np.abs(x).max()
    assert np.array_equal(got[4:], x[4:])


@pytest.mark.parametrize("B,n_mixed,C,D", [(1, 0, 1, 1), (2, 2, 1, 1), (7, 4, 30, 5), (9, 4, 65, 1), (12, 0, 6, 3), (5, 5, 4, 2)])
def test_oracle_gradients_vs_torch_autograd_fp64(B, n_mixed, C, D):
    z, d, y = _inputs(B, n_mixed, C, D, seed=B * 100 + C)
    if B > 4:
        y[-1], y[-2] = -1, C                    # clean rows without a term
    lambdas = (0.3, 1.0, 0.7)
    loss4, dz, dd = P.loss_and_grads(z, d, y, n_mixed, lambdas)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    dt = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    J, terms = P.torch_loss(zt, dt, torch.tensor(y), n_mixed, lambdas)
    J.backward()
    assert np.allclose(loss4, terms.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(dz, zt.grad.numpy(), rtol=1e-10, atol=1e-13)
    assert np.allclose(dd, dt.grad.numpy(), rtol=1e-10, atol=1e-13)
    rows = dz.sum(axis=1) + dd.sum(axis=1)
    assert np.abs(rows).max() <= 1e-14
    if B > 4 and n_mixed < B - 1:
        assert not dz[-1].any() and not dz[-2].any() and not dd[-2:].any()


def test_oracle_ties_nan_and_empty_terms():
    assert P.first_argmax([1.0, 3.0, 3.0]) == 1 and P.first_argmax([1.0, float("nan"), 9.0, float("nan")]) == 1
    z, d, y = _inputs(4, 0, 5, 3, seed=1)
    d[:, 0] = d[:, 2] = 7.0                     # tied maxima: the gradient lands on the first
    _, _, dd = P.loss_and_grads(z, d, y, 0, (1.0, 1.0, 1.0))
    assert dd[:, 0].all() and not dd[:, 1:].any()
    y[:] = -1                                   # no counting clean row, no mixed row: everything is an exact zero
    loss4, dz, dd = P.loss_and_grads(z, d, y, 0, (1.0, 1.0, 1.0))
    assert not loss4.any() and not dz.any() and not dd.any()
    z[1, 2] = np.nan
    y[:] = 0
    loss4, dz, _ = P.loss_and_grads(z, d, y, 0, (1.0, 1.0, 1.0))
    assert np.isnan(loss4[0]) and np.isnan(dz[1]).all() and np.isfinite(dz[[0, 2, 3]]).all()


def test_minus_1e9_form_equals_the_left_out_column_in_fp32():
    """The published implementations overwrite e_y with -1e9 for the third term; in fp32 exp(-1e9 - max) is an exact zero, so the value
    and the gradients are those of leaving the column out."""
    for scale in (3.0, 80.0):
        z, d, y = _inputs(9, 4, 65, 3, seed=11, scale=scale)
        outs = []
        for form in (False, True):
            zt = torch.tensor(z, requires_grad=True)
            dt = torch.tensor(d, requires_grad=True)
            J, terms = P.torch_loss(zt, dt, torch.tensor(y), 4, (0.01, 1.0, 1.0), minus_1e9=form)
            J.backward()
            outs.append((terms.detach(), zt.grad, dt.grad))
        assert torch.equal(outs[0][0][3], outs[1][0][3]), "t3 differs between the two forms"
        for a, b in zip(outs[0], outs[1]):
            assert torch.allclose(a, b, rtol=0, atol=1e-7 * scale)


def test_scores_and_bias_oracle():
    z, d, _ = _inputs(6, 0, 4, 3, seed=2)
    p = P.scores(z, d, 0.5)
    assert p.shape == (6, 5) and np.allclose(p.sum(axis=1), 1.0)
    q = P.scores(z, d + 0.5, 0.0)
    assert np.allclose(p, q)
    # floor((1 - known_rate) * n), at most n - 1
    assert [P.bias_index(n, 0.95) for n in (1, 19, 20, 39, 40, 100)] == [0, 0, 1, 1, 2, 5]
    assert P.bias_index(10, 0.5) == 5 and P.bias_index(7, 1.0) == 0 and P.bias_index(3, 0.01) == 2
    from openset_imagenet import proser
    for n in (1, 2, 19, 20, 21, 100, 1000):
        for r in (0.5, 0.9, 0.95, 0.99, 1.0):
            assert proser.bias_index(n, r) == P.bias_index(n, r)
    gt = np.array([0, 1, -1, 2, 9, 3, 1])       # C = 4: -1 and 9 take no part
    z, d, _ = _inputs(7, 0, 4, 2, seed=4)
    delta = np.sort((z.max(axis=1) - d.max(axis=1))[[0, 1, 3, 5, 6]])
    assert P.fit_bias(z, d, gt, 0.95) == float(delta[0]) and P.fit_bias(z, d, gt, 0.5) == float(delta[2])


# ---- the module on the host ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from openset_imagenet import ResNet50
    return ResNet50(10, 10, False)


def _proser(model, **kw):
    from openset_imagenet import PROSER
    kw.setdefault("generator", np.random.default_rng(0))
    return PROSER(model, **kw)


def test_construction_freezes_the_prefix_and_builds_the_dummy_classifier(model):
    p = _proser(model, dummy_count=3, mix_at="layer3")
    assert model.frozen_below == "layer3.0"
    assert tuple(p.dummy_classifier.weight.shape) == (3, 10) and tuple(p.dummy_classifier.bias.shape) == (3,)
    assert float(p.bias) == 0.0
    names = dict(model.named_parameters())
    assert not names["resnet_base.layer2.3.conv3.weight"].requires_grad and names["resnet_base.layer3.0.conv1.weight"].requires_grad
    sd = p.state_dict()
    assert "model.logits.weight" in sd and "dummy_classifier.weight" in sd and "bias" in sd
    assert sd["dummy_count"] == 3 and sd["mix_at"] == "layer3" and sd["lambdas"] == (0.01, 1.0, 1.0) and sd["alpha"] == 1.0
    q = _proser(model, dummy_count=3, mix_at="layer4")
    with torch.no_grad():
        p.bias.fill_(0.25)
    q.load_state_dict(p.state_dict())
    assert q.mix_at == "layer3" and float(q.bias) == 0.25 and torch.equal(q.dummy_classifier.weight, p.dummy_classifier.weight)
    with pytest.raises(ValueError, match="dummy_count"):
        _proser(model, dummy_count=4).load_state_dict(p.state_dict())
    with pytest.raises(ValueError, match="lacks"):
        q.load_state_dict({k: v for k, v in p.state_dict().items() if k != "alpha"})
    model.freeze_below(None)


@pytest.mark.parametrize("B", range(1, 10))
def test_draw_pairs(model, B):
    p = _proser(model, generator=np.random.default_rng(B))
    partner, weight, n_mixed = p.draw_pairs(B)
    assert n_mixed == (B // 2) & ~1 and n_mixed % 2 == 0
    assert partner.dtype == np.int32 and weight.dtype == np.float32 and partner.shape == weight.shape == (B,)
    assert P.is_involution(partner)
    assert (partner[:n_mixed] != np.arange(n_mixed)).all() and (partner[:n_mixed] < n_mixed).all()       # a perfect matching of the mixed rows
    assert (partner[n_mixed:] == np.arange(n_mixed, B)).all() and (weight[n_mixed:] == 1.0).all()        # clean rows: self-partnered, weight 1
    assert n_mixed == 0 or (0.0 <= weight[0] <= 1.0 and (weight[:n_mixed] == weight[0]).all())           # one lam per step
    again = _proser(model, generator=np.random.default_rng(B)).draw_pairs(B)
    assert np.array_equal(again[0], partner) and np.array_equal(again[1], weight)                        # reproducible from the generator
    model.freeze_below(None)


def test_draw_pairs_matchings_are_uniform(model):
    """B = 8: 4 mixed rows have 3 perfect matchings; each turns up about a third of the time."""
    p = _proser(model, generator=np.random.default_rng(123))
    seen = {}
    for _ in range(600):
        partner, _, _ = p.draw_pairs(8)
        seen[int(partner[0])] = seen.get(int(partner[0]), 0) + 1
    assert sorted(seen) == [1, 2, 3] and min(seen.values()) > 150
    model.freeze_below(None)


def test_host_refusals(model):
    from openset_imagenet import PROSER
    with pytest.raises(TypeError, match="model"):
        PROSER(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError, match="dummy_count"):
        _proser(model, dummy_count=2.0)
    with pytest.raises(TypeError, match="dummy_count"):
        _proser(model, dummy_count=True)
    with pytest.raises(ValueError, match="dummy_count"):
        _proser(model, dummy_count=0)
    with pytest.raises(ValueError, match="lambdas"):
        _proser(model, lambdas=(1.0, 1.0))
    with pytest.raises(ValueError, match="lambdas"):
        _proser(model, lambdas=(1.0, -1.0, 1.0))
    with pytest.raises(TypeError, match="lambdas"):
        _proser(model, lambdas=3)
    with pytest.raises(ValueError, match="alpha"):
        _proser(model, alpha=0.0)
    with pytest.raises(ValueError, match="alpha"):
        _proser(model, alpha=float("nan"))
    with pytest.raises(TypeError, match="generator"):
        _proser(model, generator=torch.Generator())
    with pytest.raises(ValueError, match="mix_at"):
        _proser(model, mix_at="fc")
    with pytest.raises(ValueError, match="layer9"):
        _proser(model, mix_at="layer9")
    p = _proser(model)
    with pytest.raises(TypeError, match="B"):
        p.draw_pairs(4.0)
    with pytest.raises(ValueError, match="B"):
        p.draw_pairs(0)
    z, d = np.zeros((4, 10), np.float32), np.zeros((4, 5), np.float32)
    with pytest.raises(ValueError, match="known_rate"):
        p.fit_bias(z, d, [0, 1, 2, 3], known_rate=0.0)
    with pytest.raises(ValueError, match="known_rate"):
        p.fit_bias(z, d, [0, 1, 2, 3], known_rate=1.5)
    with pytest.raises(ValueError, match="logits and dummy"):
        p.fit_bias(z[0], d, [0])
    with pytest.raises(ValueError, match="number of samples"):
        p.fit_bias(z, d[:3], [0, 1, 2, 3])
    with pytest.raises(ValueError, match="gt"):
        p.fit_bias(z, d, [0, 1, 2])
    with pytest.raises(ValueError, match="logits and dummy"):
        p.predict(z, d[0])
    with pytest.raises(ValueError, match="number of samples"):
        p.predict(z, d[:2])
    with pytest.raises(ValueError, match="at least one column"):
        p.predict(z[:, :0], d)
    with pytest.raises(ValueError, match="features"):
        p.dummy_logits(np.zeros((4, 7), np.float32))
    with pytest.raises(TypeError, match="labels"):
        p.training_step(torch.zeros(4, 3, 32, 32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="images"):
        p.training_step(torch.zeros(3, 3, 32, 32), torch.zeros(4, dtype=torch.int64))
    model.freeze_below(None)


def test_next_forward_refusals(model):
    partner, weight = torch.zeros(4, dtype=torch.int32), torch.ones(4)
    model.freeze_below(None)
    with pytest.raises(ValueError, match="frozen_below"):
        model.next_forward(mix=(partner, weight))
    model.freeze_below("fc")
    with pytest.raises(ValueError, match="frozen_below"):
        model.next_forward(mix=(partner, weight))
    model.freeze_below("layer3")
    with pytest.raises(TypeError, match="pair"):
        model.next_forward(mix=partner)
    with pytest.raises(TypeError, match="pair"):
        model.next_forward(mix=([0, 1], [1.0, 1.0]))
    with pytest.raises(TypeError, match="int32"):
        model.next_forward(mix=(partner.long(), weight))
    with pytest.raises(TypeError, match="float32"):
        model.next_forward(mix=(partner, weight.double()))
    with pytest.raises(ValueError, match="one length"):
        model.next_forward(mix=(partner, weight[:3]))
    with pytest.raises(ValueError, match="device"):
        model.next_forward(mix=(partner, weight))          # host tensors: the request takes device tensors
    assert model._fw_request is None
    model.next_forward(mix=None)
    model.freeze_below(None)


def test_no_cpu_path(model, monkeypatch):
    p = _proser(model)
    with pytest.raises(RuntimeError, match="no CPU path"):
        p(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.training_step(torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    z, d = np.zeros((4, 10), np.float32), np.zeros((4, 5), np.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.predict(z, d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.fit_bias(z, d, [0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.dummy_logits(np.zeros((4, 10), np.float32))
    model.freeze_below(None)


def test_evaluation_script_refuses_proser_under_garbage(capsys):
    from openset_imagenet.script import evaluate, proser
    with pytest.raises(SystemExit):
        evaluate.get_args(["garbage", "1", "--proser"])
    assert "--proser" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        proser.get_args(["garbage", "1"])
    args = proser.get_args(["softmax", "2", "-g", "--epochs", "2", "--dummy-count", "7"])
    assert args.epochs == 2 and args.dummy_count == 7 and args.gpu == 0 and str(args.output_directory).endswith("Protocol_2")
    assert evaluate.get_args(["entropic", "1", "--proser", "--oscr"]).proser

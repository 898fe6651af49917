"""CPU: ODIN and GradNorm (include/osi.h ABI 29, openset_imagenet/odin.py) without a GPU - the symbols and the refusals of the two ABI
calls before any launch, the host-side argument checks, the state dict, evaluate's options, and the route for models other than the
MI355X ResNet50 (autograd w.r.t. the image, adversary.pgd_step, the head restated in torch) against tests/odin_oracle.py on a small fp64
convolutional network: the literal textbook method, the sign convention and the grid search."""
import io
import math

import numpy as np
import pytest
import torch

import detection_oracle as DO
import odin_oracle as O


def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 29
    for name in ("osi_odin_head", "osi_gradnorm_scores"):
        assert hasattr(lib, name) and name in N.declared_symbols()
    import openset_imagenet
    assert openset_imagenet.ODIN is openset_imagenet.odin.ODIN and callable(openset_imagenet.odin.gradnorm_scores)


def test_abi_entries_validate_before_launch():
    """OSI_ERR_ARG (-1) and no launch: the library loads without a GPU and the pointers below are never dereferenced."""
    from openset_imagenet import _native as N
    lib = N.lib()
    a, b, c, d = 1 << 20, 2 << 20, 3 << 20, 4 << 20           # 16-byte aligned, far apart
    head = lambda logits=a, M=5, C=10, T=2.0, dlogits=b, pred=c, score=d: lib.osi_odin_head(logits, M, C, T, dlogits, pred, score, None)
    grad = lambda f=a, lg=b, M=5, F=12, C=10, T=2.0, out=c: lib.osi_gradnorm_scores(f, lg, M, F, C, T, out, None)
    bad_t = (0.0, -1.0, math.nan, math.inf)
    for kw in ([dict(logits=None), dict(score=None), dict(M=0), dict(M=-3), dict(C=0), dict(C=-1)] + [dict(T=t) for t in bad_t] +
               [dict(logits=a + 2), dict(dlogits=b + 1), dict(score=d + 2), dict(pred=c + 4), dict(dlogits=a + 8)]):
        assert head(**kw) == -1, kw
    for kw in ([dict(f=None), dict(lg=None), dict(out=None), dict(M=0), dict(F=0), dict(F=-2), dict(C=0), dict(C=-1)] +
               [dict(T=t) for t in bad_t] + [dict(f=a + 2), dict(lg=b + 1), dict(out=c + 3)]):
        assert grad(**kw) == -1, kw


def test_constructor_and_tune_refuse_bad_arguments_before_anything_runs():
    from openset_imagenet.odin import ODIN, gradnorm_scores
    assert (ODIN().temperature, ODIN().epsilon, ODIN().lo, ODIN().hi) == (1000.0, 0.0014, 0.0, 1.0)
    for kw in (dict(temperature=0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf), dict(temperature="7"),
               dict(temperature=True), dict(epsilon=-1e-3), dict(epsilon=math.inf), dict(epsilon=None), dict(lo=1.0, hi=0.0),
               dict(lo=math.nan), dict(hi="1")):
        with pytest.raises(ValueError):
            ODIN(**kw)
    odin = ODIN()
    for kw in (dict(temperatures=[], epsilons=[0.0]), dict(temperatures=[1.0], epsilons=[]), dict(temperatures=[0.0], epsilons=[0.0]),
               dict(temperatures=[1.0, math.nan], epsilons=[0.0]), dict(temperatures=[1.0], epsilons=[-0.1]), dict(temperatures=5, epsilons=[0.0]),
               dict(temperatures=[1.0], epsilons=[0.0], unk_label=0), dict(temperatures=[1.0], epsilons=[0.0], unk_label=-1.5)):
        with pytest.raises(ValueError):
            odin.tune(None, None, **kw)                      # neither the model nor the loader is looked at
    assert (odin.temperature, odin.epsilon, odin.grid.shape) == (1000.0, 0.0014, (0, 6))
    with pytest.raises(ValueError):
        odin.head(np.zeros((3,), np.float32))
    f, lg = np.ones((4, 3), np.float32), np.ones((4, 5), np.float32)
    for args in ((f, lg, 0.0), (f, lg, math.nan), (f, lg[:3], 1.0), (f[0], lg, 1.0), (f[:, :0], lg, 1.0)):
        with pytest.raises(ValueError):
            gradnorm_scores(*args)
    if not torch.cuda.is_available():                        # the checks above came first; then there is no CPU path
        with pytest.raises(RuntimeError, match="no CPU path"):
            gradnorm_scores(f, lg)
        with pytest.raises(RuntimeError, match="no CPU path"):
            odin.head(lg)


def test_state_dict_round_trip():
    from openset_imagenet.odin import GRID_COLUMNS, ODIN
    odin = ODIN(20.0, 0.002, lo=-1.0, hi=2.0)
    odin.grid = torch.arange(12, dtype=torch.float64).reshape(2, 6)
    buffer = io.BytesIO()
    torch.save(odin.state_dict(), buffer)
    buffer.seek(0)
    back = ODIN().load_state_dict(torch.load(buffer, weights_only=False))
    assert (back.temperature, back.epsilon, back.lo, back.hi) == (20.0, 0.002, -1.0, 2.0)
    assert back.grid.dtype == torch.float64 and torch.equal(back.grid, odin.grid) and len(GRID_COLUMNS) == 6
    fresh = ODIN().load_state_dict(ODIN(5.0, 0.0).state_dict())          # an untuned detector saves and loads as well
    assert (fresh.temperature, fresh.epsilon, tuple(fresh.grid.shape)) == (5.0, 0.0, (0, 6))
    sd = odin.state_dict()
    with pytest.raises(ValueError):
        ODIN().load_state_dict({k: v for k, v in sd.items() if k != "epsilon"})
    with pytest.raises(ValueError):
        ODIN().load_state_dict(dict(sd, grid=torch.zeros(2, 5)))
    with pytest.raises(ValueError):
        ODIN().load_state_dict(dict(sd, temperature=-1.0))


def test_evaluate_takes_and_refuses_the_options():
    from openset_imagenet.script.evaluate import ODIN_EPSILONS, ODIN_TEMPERATURES, get_args
    args = get_args(["softmax", "1"])
    assert (args.odin, args.odin_temperature, args.odin_epsilon, args.odin_tune, args.gradnorm, args.gradnorm_temperature) == \
        (False, 1000.0, 0.0014, False, False, 1.0)
    args = get_args(["entropic", "2", "--odin", "--odin-temperature", "10", "--odin-epsilon", "0.002", "--odin-tune", "--detection", "--gradnorm",
                     "--gradnorm-temperature", "2"])
    assert (args.odin, args.odin_temperature, args.odin_epsilon, args.odin_tune, args.gradnorm, args.gradnorm_temperature) == \
        (True, 10.0, 0.002, True, True, 2.0)
    assert ODIN_TEMPERATURES == (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000)
    assert len(ODIN_EPSILONS) == 21 and ODIN_EPSILONS[0] == 0.0 and ODIN_EPSILONS[-1] == 0.004
    assert np.allclose(np.diff(ODIN_EPSILONS), 0.0002, rtol=1e-9)
    for bad in (["garbage", "1", "--odin"], ["garbage", "1", "--detection", "--gradnorm"], ["softmax", "1", "--odin-tune"],
                ["softmax", "1", "--odin", "--odin-temperature", "0"], ["softmax", "1", "--odin", "--odin-epsilon", "-1"],
                ["softmax", "1", "--detection", "--gradnorm", "--gradnorm-temperature", "nan"], ["softmax", "1", "--gradnorm"]):
        with pytest.raises(SystemExit):
            get_args(bad)


# ------------------------------------------------------------------------------------------------- the torch restatement of the head
@pytest.mark.parametrize("T", [0.5, 1.0, 1000.0])
def test_torch_head_is_the_definition(T):
    from openset_imagenet.odin import head_reference
    x = O.head_rows(7, 10, 3).astype(np.float64)
    x[4, 2] = np.nan
    x[5, [1, 7]] = np.inf
    x[6] = -np.inf
    want_d, want_pred, want_s = O.odin_head(x, T)
    d, pred, s = head_reference(torch.from_numpy(x), T)
    assert d.dtype == torch.float64 and np.array_equal(pred.numpy(), want_pred) and want_pred[0] == 5 and want_pred[4] == 2
    assert np.allclose(d.numpy(), want_d, rtol=1e-13, atol=0, equal_nan=True) and np.allclose(s.numpy(), want_s, rtol=1e-13, atol=0, equal_nan=True)
    assert np.isnan(s.numpy()[4:]).all() and np.isnan(d.numpy()[4]).all() and np.isnan(d.numpy()[6]).all()
    if T <= 1.0:
        rest = float(d[2, [0, 1, 2, 4, 5, 6, 7, 8, 9]].sum())
        assert s[2] >= 1 - 1e-10 and d[2, 3] < 0 and abs(float(-d[2, 3]) - rest) <= 1e-12 * rest     # p_y - 1 would have cancelled
    assert head_reference(torch.from_numpy(x), T, need_grad=False)[0] is None
    one = head_reference(torch.tensor([[3.0]], dtype=torch.float32), T)
    assert one[0].dtype == torch.float32 and float(one[2]) == 1.0 and float(one[0]) == 0.0 and int(one[1]) == 0


# -------------------------------------------------------------------------------------------------- the route for any other model
class SmallNet(torch.nn.Module):
    """Three convolutions, a global mean, one linear layer; returns (logits, features) as the package's networks do. tanh: smooth, so
    that no image-gradient element is exactly zero."""

    def __init__(self, classes=10, seed=5):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.convs = torch.nn.ModuleList([torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.Conv2d(8, 8, 3, stride=2, padding=1),
                                          torch.nn.Conv2d(8, 16, 3, padding=1)])
        self.logits = torch.nn.Linear(16, classes, bias=False)
        self.double()
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.6 if p.dim() > 1 else 0.1))

    def forward(self, x):
        for conv in self.convs:
            x = torch.tanh(conv(x))
        features = x.mean((2, 3))
        return self.logits(features) * 4.0, features


SEED, EPSILON = 11, 0.05


def small_batch(seed=SEED, b=6, hw=8):
    return torch.rand(b, 3, hw, hw, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("T", [1.0, 20.0, 1000.0])
def test_generic_route_is_the_textbook_method(T):
    """ODIN.perturb / scores on a torch model in fp64 on the CPU against the literal method: x~ and the logits of x~ are EQUAL (the
    operations are the same whenever no gradient element is zero, which is asserted); `unknown` is the head's e_y / (e_y + r), the
    textbook's is torch.softmax's: the same quotient from another summation order, compared within 4 fp64 ulps."""
    from openset_imagenet.odin import ODIN
    model, x = SmallNet().train(), small_batch()
    x_t, g, unknown = O.textbook_odin(model, x, T, EPSILON)
    assert bool((g != 0).all()), "a zero gradient element: the two routes may round its sign differently; choose another seed"
    odin = ODIN(T, EPSILON)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    logits, features, got = odin.perturb(model, x)
    assert model.training and all(p.grad is None for p in model.parameters())
    assert torch.equal(got, x_t) and not torch.equal(got, x) and float((got - x).abs().max()) <= EPSILON + 1e-15
    with torch.no_grad():
        clean = model(x)
    assert torch.equal(logits, clean[0]) and torch.equal(features, clean[1]) and not logits.requires_grad
    out = odin.scores(model.eval(), x)
    assert not model.training and sorted(out) == ["features", "logits", "logits_odin", "scores", "unknown"]
    with torch.no_grad():
        assert torch.equal(out["logits_odin"], model(x_t)[0])
    assert torch.equal(out["logits"], clean[0]) and torch.equal(out["scores"], torch.softmax(clean[0], 1))
    assert out["unknown"].dtype == torch.float64 and out["unknown"].shape == (6,)
    assert float(((out["unknown"] - unknown).abs() / unknown.abs()).max()) <= 4 * 2.0 ** -52
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    # the clamp is part of the definition
    wide = ODIN(T, 0.6).perturb(model, x)[2]
    assert float(wide.min()) == 0.0 and float(wide.max()) == 1.0 and torch.equal(wide, O.textbook_odin(model, x, T, 0.6)[0])
    assert torch.equal(ODIN(T, 0.0).perturb(model, x)[2], x)


def test_sign_convention_lowers_the_loss():
    """x~ = x - epsilon sign(dJ/dx) RAISES the predicted class's probability: the batch mean of J = -log S_y(.; T) falls. A flipped
    sign raises it (checked too, so that the assertion can tell the two apart on this network)."""
    from openset_imagenet.odin import ODIN
    model, x, T = SmallNet().eval(), small_batch(), 20.0
    x_t = ODIN(T, EPSILON).perturb(model, x)[2]
    with torch.no_grad():
        j = lambda z: float(O.textbook_loss(model(z)[0], T).mean())
        flipped = torch.clamp(x + (x - x_t), 0.0, 1.0)
        assert j(x_t) < j(x) < j(flipped)


def test_mode_is_restored_after_an_exception():
    from openset_imagenet.odin import ODIN

    class Broken(ODIN):
        def _seed(self, *a):
            raise KeyError("seed")

    model = SmallNet().train()
    with pytest.raises(KeyError):
        Broken(2.0, 0.01).perturb(model, small_batch())
    assert model.training


def split(with_negatives=True, with_known=True):
    """Two batches of 8 x 8 images: known rows are smooth ramps plus a little noise, the negatives plain noise."""
    gen = torch.Generator().manual_seed(23)
    batches = []
    for b in (7, 5):
        ramp = torch.linspace(0, 1, 8, dtype=torch.float64)
        x = (ramp[None, None, :, None] * ramp[None, None, None, :]).expand(b, 3, 8, 8) * torch.rand(b, 3, 1, 1, generator=gen, dtype=torch.float64)
        x = (x + 0.05 * torch.rand(b, 3, 8, 8, generator=gen, dtype=torch.float64)).clamp(0, 1)
        y = torch.randint(0, 10, (b,), generator=gen)
        if with_negatives:
            neg = torch.arange(b) % 2 == 1
            x[neg] = torch.rand(int(neg.sum()), 3, 8, 8, generator=gen, dtype=torch.float64)
            y[neg] = -1
        if not with_known:
            y[:] = -1
        batches.append((x, y))
    return batches


def test_tune_picks_what_the_oracle_picks(monkeypatch):
    """On a host without a GPU metrics.detection_metrics has no device to count on: the numpy restatement of the same figures
    (tests/detection_oracle.py) stands in for it, for ODIN.tune and for the oracle's brute-force loop alike."""
    from openset_imagenet import odin as odin_module
    monkeypatch.setattr(odin_module.metrics, "detection_metrics", DO.metrics)
    model, batches = SmallNet(seed=9).train(), split()
    Ts, Es = (1.0, 10.0, 1000.0), (0.0, 0.01, 0.05)
    rows = O.tune(model, batches, Ts, Es, -1, DO.metrics)
    odin = odin_module.ODIN().tune(model, batches, Ts, Es, unk_label=-1)
    assert model.training and all(p.grad is None for p in model.parameters())
    assert odin.grid.shape == (9, 6) and np.array_equal(odin.grid.numpy(), np.asarray(rows, dtype=np.float64))
    best = O.pick(rows)
    assert (odin.temperature, odin.epsilon) == (best[0], best[1])
    assert len({(r[2], r[3]) for r in rows}) > 1, "every grid point scores alike: the split tells nothing"
    # the tie rules on hand-made rows: FPR, then the higher AUROC, then the smaller T, then the smaller epsilon
    made = [[10.0, 0.1, 0.5, 0.9, 0, 0], [5.0, 0.2, 0.25, 0.7, 0, 0], [5.0, 0.1, 0.25, 0.8, 0, 0], [2.0, 0.3, 0.25, 0.8, 0, 0], [2.0, 0.2, 0.25, 0.8, 0, 0]]
    assert odin_module.ODIN.select(made) == 4 and O.pick(made) == made[4]
    sd = odin_module.ODIN().load_state_dict(odin.state_dict())
    assert (sd.temperature, sd.epsilon) == (odin.temperature, odin.epsilon) and torch.equal(sd.grid, odin.grid)


def test_tune_refuses_a_split_without_negatives_or_without_known_rows(monkeypatch):
    from openset_imagenet import odin as odin_module
    monkeypatch.setattr(odin_module.metrics, "detection_metrics", DO.metrics)
    model = SmallNet(seed=9).eval()
    for batches, what in ((split(with_negatives=False), "no row labelled -1"), (split(with_known=False), "no known row"), ([], "empty")):
        odin = odin_module.ODIN(3.0, 0.01)
        with pytest.raises(ValueError, match=what):
            odin.tune(model, batches, (1.0,), (0.0, 0.01))
        assert (odin.temperature, odin.epsilon, tuple(odin.grid.shape)) == (3.0, 0.01, (0, 6)) and not model.training
    with pytest.raises(ValueError, match="no row labelled -2"):
        odin_module.ODIN().tune(model, split(), (1.0,), (0.0,), unk_label=-2)


def test_arrays_concatenate_in_order_on_the_generic_route():
    from openset_imagenet.odin import ODIN
    model, batches = SmallNet(seed=9).eval(), split()
    odin = ODIN(10.0, 0.01)
    arr = odin.arrays(model, batches)
    assert sorted(arr) == ["features", "gt", "logits", "logits_odin", "scores", "unknown"] and arr["gt"].dtype == np.float32
    assert np.array_equal(arr["gt"], np.concatenate([y.numpy() for _, y in batches]).astype(np.float32))
    second = odin.scores(model, batches[1][0])
    for k in ("logits", "features", "scores", "logits_odin", "unknown"):
        assert arr[k].shape[0] == 12 and np.array_equal(arr[k][7:], second[k].numpy()), k
    with pytest.raises(ValueError):
        odin.arrays(model, [])

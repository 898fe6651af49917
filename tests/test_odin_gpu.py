"""GPU: ODIN and GradNorm (csrc/odin.hip, include/osi.h ABI 29, openset_imagenet/odin.py).

  osi_odin_head        against the numpy fp64 restatement (tests/odin_oracle.py): score and every dlogits element within 1 fp32 ulp (fp64 on
                       both sides, sums of one sign, one rounding - the bound of osi_logit_scores), pred equal, two calls equal bits,
                       4-byte-offset buffers equal bits, either optional output left out, T = 1 the bits of OSI_SCORE_MSP, and the
                       non-finite rows as the header states them.
  osi_gradnorm_scores  |got - want| <= ulp32(want) + ||f||_1 C (C + 4) 2^-52 / T (odin_oracle.gradnorm_bound: derived, not measured).
  the torch ops        refuse wrong dtypes, devices and shapes in the shared vocabulary of csrc/osi_torch_ops.cpp.
  the MI355X route     is, bit for bit, a composition of pieces already held to fp64 elsewhere (the stance of test_adversarial_gpu.py):
                       next_backward(pgd=(-eps, inf, None), input_only=True) -> forward -> backward(head's dlogits) -> adversarial_batch(),
                       equal to pgd_step on image.grad, and it leaves the statistics, the arena, p.grad, the marks and the mode alone.
  sign convention, arrays, tune, evaluate.main."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import odin_oracle as O
import shaping_oracle as SO
from gpu_harness import Out, call, on, same_bits_nan, twice

pytestmark = pytest.mark.gpu

TEMPERATURES = (0.5, 1.0, 1000.0)


# --------------------------------------------------------------------------------------------------------------- helpers
def run_head(cuda, lg_dev, T, dlogits=True, pred=True, shift=False):
    """(dlogits or None, pred or None, score) as numpy, guard bands checked. shift: dlogits and score start 4 bytes past 16-byte
    alignment."""
    from openset_imagenet import _native as NL
    m, c = lg_dev.shape
    if shift:
        d = torch.full((m * c + 1,), 7.0, device=cuda)[1:].view(m, c) if dlogits else None
        s = torch.full((m + 1,), 7.0, device=cuda)[1:]
        p = Out((m,), torch.int64, cuda) if pred else None
        assert s.data_ptr() % 16 == 4 and (d is None or d.data_ptr() % 16 == 4)
        call(NL.lib().osi_odin_head, lg_dev, m, c, T, d, p, s)
        return (None if d is None else d.cpu().numpy()), (None if p is None else p.np()), s.cpu().numpy()
    d = Out((m, c), torch.float32, cuda) if dlogits else None
    p = Out((m,), torch.int64, cuda) if pred else None
    s = Out((m,), torch.float32, cuda)
    call(NL.lib().osi_odin_head, lg_dev, m, c, T, d, p, s)
    assert s.check() and (d is None or d.check()) and (p is None or p.check())
    return (None if d is None else d.np()), (None if p is None else p.np()), s.np()


def run_gradnorm(cuda, f_dev, lg_dev, T):
    from openset_imagenet import _native as NL
    m, f = f_dev.shape
    out = Out((m,), torch.float32, cuda)
    call(NL.lib().osi_gradnorm_scores, f_dev, lg_dev, m, f, lg_dev.shape[1], T, out)
    assert out.check()
    return out.np()


def run_msp(cuda, lg_dev):
    from openset_imagenet import _native as NL
    m, c = lg_dev.shape
    out = Out((m,), torch.float32, cuda)
    call(NL.lib().osi_logit_scores, lg_dev, m, c, NL.SCORE_MSP, out)
    return out.np()


# ---------------------------------------------------------------------------------------------------------- osi_odin_head
@pytest.mark.parametrize("c", (1, 3, 10, 64, 65, 1000, 1024, 1028, 1030))
@pytest.mark.parametrize("m", (1, 5, 67))
def test_odin_head_against_the_oracle(cuda, m, c):
    lg = O.head_rows(m, c, 100 * m + c)
    lg_dev, = on(cuda, lg)
    for T in TEMPERATURES:
        want_d, want_p, want_s = O.odin_head(lg, T)
        d, p, s = run_head(cuda, lg_dev, T)
        d2, p2, s2 = run_head(cuda, lg_dev, T)
        assert same_bits_nan(d, d2) and np.array_equal(p, p2) and same_bits_nan(s, s2), "two runs differ"
        assert p.dtype == np.int64 and np.array_equal(p, want_p), (T, p, want_p)
        assert SO.ulps(s, want_s.astype(np.float32)).max() <= 1, (T, s, want_s)
        assert SO.ulps(d, want_d.astype(np.float32)).max() <= 1, T
        if c >= 2:
            assert p[0] == c // 2                                                   # the duplicated maximum: the lowest index wins
        if m > 1 and c >= 3:
            assert p[1] == int(np.flatnonzero(lg[1] == lg[1].max())[0]) and (lg[1] == lg[1].max()).sum() == 2
        if m > 2 and T <= 1.0 and c >= 2:
            assert s[2] == 1.0 and want_s[2] >= 1 - 1e-10 and d[2, c // 3] < 0      # p_y - 1 would have cancelled to zero
        if m > 3:
            assert p[3] == 0 and SO.ulps(s[3:4], np.float32([1.0 / c])).max() <= 1
        if c == 1:
            assert (s == 1.0).all() and (d == 0.0).all() and (p == 0).all()
        # each optional output alone: the others keep their bits
        _, p3, s3 = run_head(cuda, lg_dev, T, dlogits=False)
        d4, _, s4 = run_head(cuda, lg_dev, T, pred=False)
        assert np.array_equal(p3, p) and same_bits_nan(s3, s) and same_bits_nan(d4, d) and same_bits_nan(s4, s)
        # rows and outputs 4 bytes past 16-byte alignment: the same order, the same bits
        shifted = torch.zeros(m * c + 1, dtype=torch.float32, device=cuda)[1:].view(m, c)
        shifted.copy_(lg_dev)
        d5, p5, s5 = run_head(cuda, shifted, T, shift=True)
        assert shifted.data_ptr() % 16 == 4 and same_bits_nan(d5, d) and np.array_equal(p5, p) and same_bits_nan(s5, s)
        if T == 1.0:
            assert same_bits_nan(s, run_msp(cuda, lg_dev)) and same_bits_nan(s5, run_msp(cuda, shifted))


@pytest.mark.parametrize("c", (5, 8, 1030))
def test_odin_head_non_finite_rows(cuda, c):
    """As include/osi.h states them: a NaN in a row gives NaN everywhere and pred = the first NaN's column; a +Inf maximum is not
    subtracted, so the score is NaN as under OSI_SCORE_MSP, dlogits 0 in the finite columns and -0 (one +Inf) or NaN (several) at the
    +Inf columns; a row of -Inf gives NaN, NaN and pred 0."""
    rng = np.random.default_rng(c)
    lg = rng.standard_normal((6, c)).astype(np.float32)
    lg[0, [3, 1]] = np.nan
    lg[1, 2] = np.inf
    lg[2, [4, 2]] = np.inf
    lg[3] = -np.inf
    lg[4, c - 1] = np.nan                                     # the last column, owned by another lane than the maximum
    lg[4, 0] = 50.0
    lg[5, 1] = -np.inf                                        # harmless: exp = 0
    lg_dev, = on(cuda, lg)
    for T in TEMPERATURES:
        want_d, want_p, want_s = O.odin_head(lg, T)
        d, p, s = twice_head(cuda, lg_dev, T)
        assert np.array_equal(p, want_p) and list(p[:5]) == [1, 2, 2, 0, c - 1]
        assert SO.ulps(s, want_s.astype(np.float32)).max() <= 1 and SO.ulps(d, want_d.astype(np.float32)).max() <= 1
        assert np.isnan(s[:5]).all() and np.isfinite(s[5]) and np.isnan(d[0]).all() and np.isnan(d[3]).all() and np.isnan(d[4]).all()
        finite = np.isfinite(lg[1])
        assert (d[1][finite] == 0).all() and d[1, 2] == 0 and np.signbit(d[1, 2])
        assert np.isnan(d[2, [2, 4]]).all() and (d[2][np.isfinite(lg[2])] == 0).all()
        assert d[5, 1] == 0 and np.isfinite(d[5]).all()
        if T == 1.0:
            assert same_bits_nan(s, run_msp(cuda, lg_dev))


def twice_head(cuda, lg_dev, T):
    d = twice(lambda: run_head(cuda, lg_dev, T)[0])
    _, p, s = run_head(cuda, lg_dev, T)
    return d, p, s


# ----------------------------------------------------------------------------------------------------- osi_gradnorm_scores
@pytest.mark.parametrize("c", (3, 1000, 1030))
@pytest.mark.parametrize("f", (1, 12, 2048))
@pytest.mark.parametrize("m", (1, 67))
def test_gradnorm_against_the_oracle(cuda, m, f, c):
    rng = np.random.default_rng(1000 * m + 10 * f + c)
    feats = rng.standard_normal((m, f)).astype(np.float32)                 # both signs: the L1 norm takes no sign for granted
    lg = (3.0 * rng.standard_normal((m, c))).astype(np.float32)
    lg[0] = np.float32(0.25)                                                # a uniform row: every |C p - 1| cancels to (about) zero
    if m > 2:
        lg[1, c // 2] = np.float32(70.0)                                    # one dominant logit: the sum is 2 (C - 1) / C ... 2
        feats[2] = -np.abs(feats[2])
    assert (feats < 0).any() and (feats > 0).any() or f == 1
    f_dev, lg_dev = on(cuda, feats, lg)
    for T in TEMPERATURES:
        want = O.gradnorm(feats, lg, T)
        got = twice(lambda: run_gradnorm(cuda, f_dev, lg_dev, T))
        bound = O.gradnorm_bound(feats, lg, T, want)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), (T, got, want, bound)
        assert got[0] <= bound[0] and (got >= 0).all()
        fs = torch.zeros(m * f + 1, dtype=torch.float32, device=cuda)[1:].view(m, f)
        ls = torch.zeros(m * c + 1, dtype=torch.float32, device=cuda)[1:].view(m, c)
        fs.copy_(f_dev), ls.copy_(lg_dev)
        assert fs.data_ptr() % 16 == 4 and same_bits_nan(run_gradnorm(cuda, fs, ls, T), got)
    nan_f, nan_l, inf_l = feats.copy(), lg.copy(), lg.copy()
    nan_f[0, f - 1], nan_l[0, c - 1], inf_l[0, 0] = np.nan, np.nan, np.inf
    for a, b in ((nan_f, lg), (feats, nan_l), (feats, inf_l)):
        got = run_gradnorm(cuda, *on(cuda, a, b), 2.0)
        assert np.isnan(got[0]) and np.isfinite(got[1:]).all()


# ----------------------------------------------------------------------------------------------------------- the torch ops
def test_torch_ops_answer_and_refuse(cuda):
    from openset_imagenet import _native as NL
    from openset_imagenet.odin import ODIN, gradnorm_scores
    ops = NL.ops()
    lg = O.head_rows(9, 10, 1)
    feats = np.random.default_rng(2).standard_normal((9, 12)).astype(np.float32)
    lg_dev, f_dev = on(cuda, lg, feats)
    d, p, s = ops.odin_head(lg_dev, 2.0, True)
    want = run_head(cuda, lg_dev, 2.0)
    assert same_bits_nan(d.cpu().numpy(), want[0]) and np.array_equal(p.cpu().numpy(), want[1]) and same_bits_nan(s.cpu().numpy(), want[2])
    assert torch.equal(p, lg_dev.argmax(1))
    d0, p0, s0 = ops.odin_head(lg_dev, 2.0, False)
    assert d0.numel() == 0 and torch.equal(p0, p) and torch.equal(s0, s)
    hd, hp, hs = ODIN(2.0).head(lg)
    assert torch.equal(hd, d) and torch.equal(hp, p) and torch.equal(hs, s)
    g = ops.gradnorm_scores(f_dev, lg_dev, 2.0)
    assert same_bits_nan(g.cpu().numpy(), run_gradnorm(cuda, f_dev, lg_dev, 2.0)) and torch.equal(gradnorm_scores(feats, lg, 2.0), g)
    assert torch.equal(ops.odin_head(lg_dev[3:], 2.0, True)[2], s[3:])                        # a row slice: 8 bytes past 16
    refusals = (
        (lambda: ops.odin_head(lg_dev.double(), 2.0, True), "osi::odin_head: logits has dtype"),
        (lambda: ops.odin_head(lg_dev[0], 2.0, True), "osi::odin_head: logits"),
        (lambda: ops.odin_head(lg_dev[:, ::2], 2.0, True), "osi::odin_head: logits must be contiguous"),
        (lambda: ops.odin_head(lg_dev[:0], 2.0, True), "osi::odin_head: sizes out of range"),
        (lambda: ops.odin_head(lg_dev, 0.0, True), "osi_odin_head failed: invalid"),
        (lambda: ops.odin_head(lg_dev, math.nan, True), "osi_odin_head failed: invalid"),
        (lambda: ops.gradnorm_scores(f_dev.half(), lg_dev, 1.0), "osi::gradnorm_scores: features has dtype"),
        (lambda: ops.gradnorm_scores(f_dev, lg_dev.double(), 1.0), "osi::gradnorm_scores: logits has dtype"),
        (lambda: ops.gradnorm_scores(f_dev, lg_dev.cpu(), 1.0), "osi::gradnorm_scores: logits must live on the GPU"),
        (lambda: ops.gradnorm_scores(f_dev[:8], lg_dev, 1.0), "osi::gradnorm_scores: tensors disagree on the number of rows"),
        (lambda: ops.gradnorm_scores(f_dev.view(-1), lg_dev, 1.0), "osi::gradnorm_scores: features"),
        (lambda: ops.gradnorm_scores(f_dev, lg_dev, -1.0), "osi_gradnorm_scores failed: invalid"),
    )
    for run, match in refusals:
        with pytest.raises(RuntimeError, match=match):
            run()
    with pytest.raises(RuntimeError):                         # a CPU reference tensor finds no kernel under the HIP key
        ops.odin_head(lg_dev.cpu(), 2.0, True)
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------- the MI355X route
B, HW, C = 8, 64, 10
MODEL_SEED, IMAGE_SEED = 91, 93
T_NET, EPS_NET = 1000.0, 0.0014                               # the defaults


def _model(cuda, seed=MODEL_SEED):
    from openset_imagenet import ResNet50
    from oracle import resnet50_oracle as R
    gen = torch.Generator().manual_seed(seed)
    sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), generator=gen)
    model = ResNet50(C, C, False)
    model.load_state_dict(sd)
    return model.to(cuda).train()


def _images(cuda, b=B, seed=IMAGE_SEED):
    return torch.rand(b, 3, HW, HW, generator=torch.Generator().manual_seed(seed)).to(cuda)


def _nhwc4(x):
    from openset_imagenet.adversary import as_nhwc4
    return as_nhwc4(x)


def _hand(model, images, T, eps):
    """The hand-written sequence of the issue, in eval mode."""
    from openset_imagenet import _native as NL
    model.eval()
    model.next_backward(pgd=(-eps, math.inf, None), lo=0.0, hi=1.0, input_only=True)
    with torch.enable_grad():
        logits, features = model(images)
        logits.backward(NL.ops().odin_head(logits.detach(), T, True)[0])
    return logits.detach().clone(), features.detach().clone(), model.adversarial_batch().clone()


def test_perturb_is_the_hand_written_sequence_and_leaves_the_model_alone(cuda):
    from openset_imagenet import _native as NL
    from openset_imagenet.adversary import pgd_step
    from openset_imagenet.odin import ODIN
    model, x = _model(cuda), _images(cuda)
    odin = ODIN(T_NET, EPS_NET)
    u8 = (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    gen = torch.Generator().manual_seed(5)
    sentinel = torch.randn(model._flat_grads.shape, generator=gen).to(cuda)
    with torch.no_grad():
        model._flat_grads.copy_(sentinel)
    model.bind_gradients()
    grads_before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert len(grads_before) == 162
    for fresh, training in ((False, True), (True, False)):
        model.train(training)
        model._grads_fresh = fresh
        bufs, nbt = model._flat_buffers.clone(), model._nbt.clone()
        for images in (x, _nhwc4(x), u8):
            want = _hand(model, images, T_NET, EPS_NET)
            model.train(training)
            logits, features, x_t = odin.perturb(model, images)
            torch.cuda.synchronize()
            assert x_t.shape == (B, HW, HW, 4) and x_t.data_ptr() == model.adversarial_batch().data_ptr()
            assert torch.equal(logits, want[0]) and torch.equal(features, want[1]) and torch.equal(x_t, want[2])
            assert not torch.equal(x_t, _nhwc4(images)) and float((x_t - _nhwc4(images)).abs().max()) <= EPS_NET + 1e-7
            assert model.training is training and model._bw_request is None and model._grads_fresh is fresh and not model.bn_frozen
            assert torch.equal(model._flat_buffers, bufs) and torch.equal(model._nbt, nbt) and torch.equal(model._flat_grads, sentinel)
            assert all(torch.equal(p.grad, grads_before[n]) for n, p in model.named_parameters())
            assert all(p.requires_grad for p in model.parameters())
        # tune's path: the dJ/dimage route, then pgd_step
        clean = _nhwc4(x)[..., :3].permute(0, 3, 1, 2).contiguous()
        grad = odin._image_grad(model.eval(), model, clean, T_NET)
        model.train(training)
        assert torch.equal(_nhwc4(pgd_step(clean, grad, clean, -EPS_NET, math.inf)), odin.perturb(model, x)[2])
        assert torch.equal(model._flat_grads, sentinel) and model._grads_fresh is fresh and all(p.requires_grad for p in model.parameters())
        assert torch.equal(model._flat_buffers, bufs) and torch.equal(model._nbt, nbt)
        # scores(): minus the head's score of a plain no-grad forward on x~
        clean_logits, clean_features, _ = _hand(model, x, T_NET, EPS_NET)
        model.train(training)
        out = odin.scores(model, x)
        x_t = model.adversarial_batch().clone()
        model.eval()
        with torch.no_grad():
            plain = model(x_t)[0]
        model.train(training)
        assert torch.equal(out["logits_odin"], plain) and torch.equal(out["unknown"], -NL.ops().odin_head(plain, T_NET, False)[2])
        assert torch.equal(out["logits"], clean_logits) and torch.equal(out["features"], clean_features)      # the clean forward's
        assert torch.equal(out["scores"], NL.ops().softmax(clean_logits)) and out["unknown"].shape == (B,)
        assert model.training is training and torch.equal(model._flat_buffers, bufs) and torch.equal(model._nbt, nbt)
    # a second batch of another size
    x3 = _images(cuda, 3, 7)
    want = _hand(model, x3, T_NET, EPS_NET)
    assert torch.equal(odin.perturb(model, x3)[2], want[2]) and odin.scores(model, x3)["unknown"].shape == (3,)
    # behind a wrapper that holds the network as .module (data parallel): the same route, the wrapper's mode restored as well
    class Wrapped(torch.nn.Module):
        def __init__(self, module):
            super().__init__()
            self.module = module

        def forward(self, *a, **k):
            return self.module(*a, **k)

    wrapped = Wrapped(model).train()
    want = _hand(model, x, T_NET, EPS_NET)
    wrapped.train()
    assert torch.equal(odin.perturb(wrapped, x)[2], want[2]) and wrapped.training and model.training and model._bw_request is None
    model.eval()
    # epsilon = 0: the clean batch
    assert torch.equal(ODIN(T_NET, 0.0).perturb(model, x)[2], _nhwc4(x))
    assert torch.equal(model._flat_grads, sentinel)


def test_an_exception_inside_leaves_no_request_and_restores_the_mode(cuda):
    from openset_imagenet import tools
    from openset_imagenet.odin import ODIN
    tools.set_device_gpu(0)

    class Broken(ODIN):
        def _seed(self, *a):
            raise KeyError("seed")

    model, x = _model(cuda), _images(cuda, 3, 7)
    for training in (True, False):
        model.train(training)
        for call_ in (lambda o: o.perturb(model, x), lambda o: o.scores(model, x), lambda o: o.tune(model, [(x, torch.tensor([0, -1, 1]))], [1.0], [0.0])):
            with pytest.raises(KeyError):
                call_(Broken(2.0, 0.01))
            assert model.training is training and model._bw_request is None and all(p.requires_grad for p in model.parameters())
    good = ODIN(2.0, 0.01).perturb(model, x)[2]               # and the next call works
    assert good.shape == (3, HW, HW, 4)
    model.freeze_below("layer2")
    with pytest.raises(ValueError, match="freeze_below"):
        ODIN().perturb(model, x)
    with pytest.raises(ValueError, match="freeze_below"):
        ODIN().tune(model, [(x, torch.tensor([0, -1, 1]))], [1.0], [0.0])
    model.freeze_below(None)


def test_sign_convention_on_the_network(cuda):
    """Model seed 91 (oracle init_state + randomize_bn, C = 10), images seed 93 (B = 8, 64 x 64), T = 1000, epsilon = 0.0014: the fp64
    CPU oracle (oracle/resnet50_oracle.py, eval mode) gives a batch mean of J = -log S_y(.; T) of 2.2010978 at x and 2.1996992 at x~ -
    it falls, for every one of the 8 rows, and no element of the oracle's image gradient is zero. Here both are read off the head's
    score; a flipped sign would raise J."""
    from openset_imagenet import _native as NL
    from openset_imagenet.odin import ODIN
    model, x = _model(cuda).eval(), _images(cuda)
    out = ODIN(T_NET, EPS_NET).scores(model, x)
    j_clean = -torch.log(NL.ops().odin_head(out["logits"], T_NET, False)[2].double())
    j_odin = -torch.log((-out["unknown"]).double())
    print(f"J(x) = {float(j_clean.mean()):.7f}, J(x~) = {float(j_odin.mean()):.7f}")
    assert float(j_odin.mean()) < float(j_clean.mean()) and bool((j_odin < j_clean).all())
    assert abs(float(j_clean.mean()) - 2.2010978) < 1e-3 and abs(float(j_odin.mean()) - 2.1996992) < 1e-3
    flipped = ODIN(T_NET, EPS_NET)
    flipped._seed = lambda logits, features, T, kernel: (-ODIN._seed(flipped, logits, features, T, kernel)[0], None)
    j_flip = -torch.log((-flipped.scores(model, x)["unknown"]).double())
    assert float(j_flip.mean()) > float(j_clean.mean())


# ------------------------------------------------------------------------------------------------------- arrays and tune
def _loader(cuda):
    gen = torch.Generator().manual_seed(17)
    batches = []
    for _ in range(2):
        x = torch.rand(B, 3, HW, HW, generator=gen)
        y = torch.randint(0, C, (B,), generator=gen)
        y[1::3] = -1
        x[1::3] = torch.rand(int((y == -1).sum()), 3, 1, 1, generator=gen).expand(-1, 3, HW, HW) * 0.5 + 0.25   # flat grey negatives
        batches.append((x, y))
    return batches


def test_arrays_and_tune(cuda):
    from openset_imagenet import _native as NL, metrics, tools
    from openset_imagenet.odin import ODIN
    tools.set_device_gpu(0)
    model, loader = _model(cuda).eval(), _loader(cuda)
    gt = np.concatenate([y.numpy() for _, y in loader])
    assert set(gt.tolist()) <= set(range(-1, C)) and (gt == -1).sum() == 6
    odin = ODIN(20.0, 0.002)
    arr = odin.arrays(model, loader)
    assert sorted(arr) == ["features", "gt", "logits", "logits_odin", "scores", "unknown"]
    assert arr["gt"].dtype == np.float32 and np.array_equal(arr["gt"], gt.astype(np.float32))
    for i, (x, _) in enumerate(loader):                       # the rows concatenate in order
        out = odin.scores(model, x.to(cuda))
        for k in ("logits", "features", "scores", "logits_odin", "unknown"):
            assert arr[k].dtype == np.float32 and np.array_equal(arr[k][B * i:B * (i + 1)], out[k].cpu().numpy()), k
    assert np.isfinite(arr["unknown"]).all() and (arr["unknown"] < 0).all() and (arr["unknown"] >= -1).all()
    # tune = the brute-force loop over ODIN(T, eps).arrays
    Ts, Es = (1.0, 100.0), (0.0, 0.003)
    rows = []
    for T in Ts:
        for eps in Es:
            m = metrics.detection_metrics(gt, ODIN(T, eps).arrays(model, loader)["unknown"], unk_label=-1, tpr=(0.95,))
            rows.append([T, eps, m["fpr_at_tpr"][0], m["auroc"], m["aupr_in"], m["aupr_out"]])
    # one backward's dgrad ops, then tune's: |T| backwards per batch and no weight-gradient op
    lib = NL.lib()
    net = model._last[0]
    ms, ops = (ctypes.c_double * 7)(), (ctypes.c_int * 7)()
    sentinel = model._flat_grads.fill_(4321.0).clone()
    NL.check(lib.osi_resnet50_profile(net.h, 1), "profile on")
    try:
        odin._image_grad(model, model, loader[0][0].to(cuda), 20.0)           # one backward of tune's route
        NL.check(lib.osi_resnet50_profile_read(net.h, ms, ops), "profile_read")
        one = ops[2]
        tuned = ODIN().tune(model, loader, Ts, Es, unk_label=-1)
        NL.check(lib.osi_resnet50_profile_read(net.h, ms, ops), "profile_read")
    finally:
        NL.check(lib.osi_resnet50_profile(net.h, 0), "profile off")
    torch.cuda.synchronize()
    assert one > 0 and ops[2] == len(loader) * len(Ts) * one, (one, ops[2])      # OSI_PROF_CONV_DGRAD
    assert ops[3] == 0 and torch.equal(model._flat_grads, sentinel)              # OSI_PROF_CONV_WGRAD
    assert np.array_equal(tuned.grid.numpy(), np.asarray(rows, dtype=np.float64))
    best = O.pick(rows)
    assert (tuned.temperature, tuned.epsilon) == (best[0], best[1]) and not model.training
    with pytest.raises(ValueError, match="no row labelled -2"):
        ODIN().tune(model, loader, Ts, Es, unk_label=-2)


# ------------------------------------------------------------------------------------------------------------ evaluate.py
def test_evaluate_main_writes_the_odin_arrays_and_the_detection_rows(cuda, tmp_path, monkeypatch):
    """script/evaluate.py end to end on four JPEGs a split, the grid of --odin-tune cut to 2 x 2."""
    from PIL import Image
    from openset_imagenet import ResNet50, tools
    from openset_imagenet.odin import ODIN
    from openset_imagenet.script import evaluate
    tools.set_device_gpu(0)
    rng = np.random.default_rng(0)
    img_dir, proto, out = tmp_path / "imgs", tmp_path / "protocols", tmp_path / "out"
    for d in (img_dir, proto, out):
        d.mkdir()
    labels = {"val": (0, 1, 2, -1), "test": (2, -2, 0, -1)}
    for split, ys in labels.items():
        for i, y in enumerate(ys):
            Image.fromarray(rng.integers(0, 256, size=(256, 256, 3), dtype=np.uint8)).save(img_dir / f"{split}_{i}.jpg", quality=90)
        (proto / f"p2_{split}.csv").write_text("".join(f"{split}_{i}.jpg,{y}\n" for i, y in enumerate(ys)))
    torch.manual_seed(3)
    torch.save({"epoch": 1, "model_state_dict": ResNet50(3, 3, False).state_dict(), "opt_state_dict": {}, "best_score": 0.5},
               out / "softmax_curr.pth")
    base = ["softmax", "2", "-g", "0", "--imagenet-directory", str(img_dir), "--protocol-directory", str(proto), "--output-directory",
            str(out), "--batch-size", "4", "--workers", "0"]
    plain = {k: dict(np.load(v)) for k, v in evaluate.main(base).items()}
    monkeypatch.setattr(evaluate, "ODIN_TEMPERATURES", (1, 1000))
    monkeypatch.setattr(evaluate, "ODIN_EPSILONS", (0.0, 0.002))
    written = evaluate.main(base + ["--odin", "--odin-tune", "--oscr", "--detection", "--gradnorm", "--gradnorm-temperature", "2"])
    assert sorted(written) == ["test", "test_detection", "test_odin", "val", "val_detection", "val_odin"]
    restored = ODIN().load_state_dict(torch.load(out / "softmax_odin_curr.pth", weights_only=False))
    assert restored.grid.shape == (4, 6) and restored.temperature in (1.0, 1000.0) and restored.epsilon in (0.0, 0.002)
    for split in ("val", "test"):
        a = dict(np.load(written[f"{split}_odin"]))
        assert sorted(a) == ["features", "gt", "logits", "logits_odin", "scores", "unknown"]
        for key in ("gt", "logits", "features", "scores"):   # the plain files are what they are without the options
            assert np.array_equal(dict(np.load(written[split]))[key], plain[split][key]), key
            # ODIN's own clean forward is the differentiable one on the running statistics: the inference forward's values up to fp32 rounding
            assert a[key].dtype == plain[split][key].dtype and np.allclose(a[key], plain[split][key], rtol=1e-4, atol=1e-4), key
        assert np.array_equal(a["gt"], plain[split]["gt"])
        assert a["logits_odin"].shape == (4, 3) and a["unknown"].shape == (4,) and np.isfinite(a["unknown"]).all()
        assert (a["unknown"] < 0).all() and (a["unknown"] >= -1).all()
        rows = json.load(open(written[f"{split}_detection"]))["rows"]
        scorers = [r["scorer"] for r in rows if r["unk_label"] == -1]
        assert scorers == ["MSP", "MaxLogit", "Energy", "GradNorm", "ODIN"]
        assert all("error" not in r and 0.0 <= r["auroc"] <= 1.0 for r in rows)

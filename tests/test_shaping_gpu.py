"""GPU parity of activation shaping (csrc/shaping.hip, openset_imagenet/shaping.py) against the numpy fp64 oracle of
tests/shaping_oracle.py: every call through the C ABI on identical input bits, with 256-byte guard bands around every output and a fresh
workspace full of 0xFF bytes for every call, every call twice with equal bits; then the pooled accessor of the executor and the whole
of ActivationShaping.

Every bound is derived, none measured:
  order_stats   no arithmetic: bit-equal to the oracle's stable sort (a NaN compared as a NaN).
  REACT, ASH_P  no arithmetic but a select: bit-equal.
  ASH_B         the support is the oracle's kept set exactly (this is how the tie rule is checked); the fill (float)(s1 / keep) within
                1 fp32 ulp: the two fp64 sums differ by at most (F + 2) 2^-53 relative, which can move the rounding by one ulp.
  ASH_S, SCALE  within 2 fp32 ulp on non-negative input: the same difference of the sums (all terms of one sign: no cancellation) can
                move the rounded factor exp(s1 / s2) by one fp32 ulp (s1 / s2 <= F / keep here, so the exponential amplifies the
                relative error by at most a few thousand: far below 2^-24), and the fp32 product rounds once more.
  logit_scores  fp64 on both sides, row sums of C terms of one sign: within 1 fp32 ulp after the one rounding.
  clip          two exact order statistics, interpolated in fp64 by the same rule as numpy: within 1 fp32 ulp of np.percentile."""
import ctypes

import numpy as np
import pytest
import torch

import shaping_oracle as O
from gpu_harness import Out, call, poisoned, same_bits_nan, twice

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------------------- helpers
def run_order_stats(cuda, v_dev, n, ranks):
    from openset_imagenet import _native as NL
    lib = NL.lib()
    nb = lib.osi_order_stats_workspace(n, len(ranks))
    out = Out((len(ranks),), torch.float32, cuda)
    call(lib.osi_order_stats_f32, v_dev, n, (ctypes.c_longlong * len(ranks))(*ranks), len(ranks), out, poisoned(nb, cuda), nb)
    assert out.check()
    return out.np()


def run_shape_rows(cuda, x_dev, mode, keep, clip=0.0):
    from openset_imagenet import _native as NL
    lib = NL.lib()
    m, f = x_dev.shape
    nb = lib.osi_shape_rows_workspace(m, f)
    out = Out((m, f), torch.float32, cuda)
    call(lib.osi_shape_rows, x_dev, m, f, mode, keep, float(clip), out, poisoned(nb, cuda), nb)
    assert out.check()
    return out.np()


def run_logit_scores(cuda, lg_dev, mode):
    from openset_imagenet import _native as NL
    m, c = lg_dev.shape
    out = Out((m,), torch.float32, cuda)
    call(NL.lib().osi_logit_scores, lg_dev, m, c, mode, out)
    assert out.check()
    return out.np()


# ----------------------------------------------------------------------------------------------------------- order_stats
@pytest.mark.parametrize("name", O.STATS_DATA)
@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 65537, 1000003))
def test_order_stats_against_the_stable_sort(cuda, n, name):
    v = O.stats_data(name, n)
    lead = n % 4                                            # floats between a 16-byte boundary and v[0]: every head / tail length
    buf = torch.zeros(n + 8, dtype=torch.float32, device=cuda)
    v_dev = buf[lead:lead + n]
    v_dev.copy_(torch.from_numpy(v))
    assert v_dev.data_ptr() % 16 == 4 * lead and same_bits_nan(v_dev.cpu().numpy(), v)
    mid = (n - 1) // 2
    ranks = [0, n - 1, mid, min(mid + 1, n - 1), mid]       # the ends, an adjacent pair in the middle, a duplicate
    got = twice(lambda: run_order_stats(cuda, v_dev, n, ranks))
    want = O.order_stats(v, ranks)
    assert same_bits_nan(got, want), (got, want)
    assert not np.signbit(got[got == 0]).any()              # a zero comes back as +0
    if n >= 8:                                              # eight ranks in no order, one launch
        ranks = [n - 1, 0, n // 3, n // 3 + 1, n - 2, 1, n // 2, n // 7]
        assert same_bits_nan(twice(lambda: run_order_stats(cuda, v_dev, n, ranks)), O.order_stats(v, ranks))


def test_order_stats_returns_canonical_zero(cuda):
    v = np.array([-0.0, -0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    got = run_order_stats(cuda, torch.from_numpy(v).to(cuda), 5, [1, 2, 3])
    assert got.tolist() == [0.0, 0.0, 0.0] and not np.signbit(got).any()


# ------------------------------------------------------------------------------------------------------------ shape_rows
def keeps_of(f):
    return sorted({k for k in (1, 2, f - 1, f, O.keep_of(f, 90.0)) if 1 <= k <= f})


@pytest.mark.parametrize("f", (1, 2, 63, 64, 65, 257, 2048, 4095, 4096))
@pytest.mark.parametrize("m", (1, 3, 65))
def test_shape_rows_against_the_oracle(cuda, m, f):
    x = O.relu_rows(m, f, seed=1000 * m + f)
    x_dev = torch.from_numpy(x).to(cuda)
    clip = float(np.float32(0.75))                          # a value the rows hold: x > clip is false on the duplicates
    got = twice(lambda: run_shape_rows(cuda, x_dev, O.REACT, 0, clip))
    assert same_bits_nan(got, O.shape_rows(x, O.REACT, 0, clip)[0])
    shifted = torch.zeros(m * f + 1, dtype=torch.float32, device=cuda)[1:].view(m, f)        # 4-byte aligned only: the scalar form
    shifted.copy_(x_dev)
    assert shifted.data_ptr() % 16 == 4 and same_bits_nan(run_shape_rows(cuda, shifted, O.REACT, 0, clip), got)
    filled = 0
    for keep in keeps_of(f):
        kept = O.kept_masks(x, keep)
        want, mask = O.shape_rows(x, O.ASH_P, keep, kept=kept)
        assert mask.sum(axis=1).tolist() == [keep] * m
        got = twice(lambda: run_shape_rows(cuda, x_dev, O.ASH_P, keep))
        assert same_bits_nan(got, want), (keep, "ash_p")
        want, mask = O.shape_rows(x, O.ASH_B, keep, kept=kept)
        got = twice(lambda: run_shape_rows(cuda, x_dev, O.ASH_B, keep))
        assert np.array_equal(got != 0, want != 0), (keep, "ash_b support")          # the oracle's kept set wherever the fill is not 0
        rows = want.max(axis=1) > 0
        assert np.array_equal((got != 0)[rows], mask[rows])
        filled += int(rows.sum())
        assert O.ulps(got, want).max() <= 1, (keep, "ash_b fill")
        for mode in (O.ASH_S, O.SCALE):
            want, _ = O.shape_rows(x, mode, keep, kept=kept)
            got = twice(lambda: run_shape_rows(cuda, x_dev, mode, keep))
            assert O.ulps(got, want).max() <= 2, (keep, mode, int(O.ulps(got, want).max()))
    assert filled > 0 or f <= 2


def test_shape_rows_orders_nan_and_inf(cuda):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((5, 300)).astype(np.float32)
    pick = rng.random(x.shape)
    for lo, value in ((0.0, np.nan), (0.05, np.inf), (0.1, -np.inf), (0.15, -0.0), (0.2, 0.0)):
        x[(pick >= lo) & (pick < lo + 0.05)] = value
    x[4] = np.nan                                           # every column ties: the lowest stay
    x_dev = torch.from_numpy(x).to(cuda)
    for keep in (1, 7, 16, 40, 150, 299, 300):              # inside the NaNs, inside the Infs, among the zeros of both signs
        want, mask = O.shape_rows(x, O.ASH_P, keep)
        got = twice(lambda: run_shape_rows(cuda, x_dev, O.ASH_P, keep))
        assert same_bits_nan(got, want), keep
        assert np.isnan(got[4, :keep]).all() and (got[4, keep:] == 0).all()


# ---------------------------------------------------------------------------------------------------------- logit_scores
@pytest.mark.parametrize("c", (1, 2, 7, 64, 65, 1000))
@pytest.mark.parametrize("m", (1, 5, 257))
def test_logit_scores_against_the_oracle(cuda, m, c):
    rng = np.random.default_rng(100 * m + c)
    lg = (rng.standard_normal((m, c)) * 30).astype(np.float32)
    lg[rng.random((m, c)) < 0.1] = np.float32(80.0)         # an unshifted fp32 exp overflows
    lg[rng.random((m, c)) < 0.1] = np.float32(-80.0)
    lg[rng.random((m, c)) < 0.05] = -np.inf
    if m > 1:
        lg[1] = -np.inf                                     # -Inf, -Inf, NaN
    lg_dev = torch.from_numpy(lg).to(cuda)
    for mode in (O.ENERGY, O.MAXLOGIT, O.MSP):
        got = twice(lambda: run_logit_scores(cuda, lg_dev, mode))
        want = O.logit_scores(lg, mode).astype(np.float32)
        assert O.ulps(got, want).max() <= 1, (mode, got, want)
        shifted = torch.zeros(m * c + 1, dtype=torch.float32, device=cuda)[1:].view(m, c)    # 4-byte aligned rows: the same order, the same bits
        shifted.copy_(lg_dev)
        assert shifted.data_ptr() % 16 == 4 and same_bits_nan(run_logit_scores(cuda, shifted, mode), got)
    if m > 1:
        e, mx, p = (run_logit_scores(cuda, lg_dev, mode)[1] for mode in (O.ENERGY, O.MAXLOGIT, O.MSP))
        assert e == -np.inf and mx == -np.inf and np.isnan(p)


def test_logit_scores_propagate_nan_and_plus_inf(cuda):
    lg = np.array([[1, np.nan, 2], [np.inf, 0, 1], [np.nan] * 3], dtype=np.float32)
    lg_dev = torch.from_numpy(lg).to(cuda)
    for mode in (O.ENERGY, O.MAXLOGIT, O.MSP):
        got = run_logit_scores(cuda, lg_dev, mode)
        assert same_bits_nan(np.isnan(got).astype(np.float32), np.isnan(O.logit_scores(lg, mode)).astype(np.float32)), mode
        assert np.isnan(got[0]) and np.isnan(got[2])
    assert run_logit_scores(cuda, lg_dev, O.ENERGY)[1] == np.inf and run_logit_scores(cuda, lg_dev, O.MAXLOGIT)[1] == np.inf


# ------------------------------------------------------------------------------------------------------- pooled accessor
def test_pooled_is_the_input_of_the_head(cuda):
    from openset_imagenet import ResNet50, tools, _native as NL
    from openset_imagenet.shaping import head_of
    from openset_imagenet.train import get_arrays
    tools.set_device_gpu(0)
    torch.manual_seed(0)
    model = tools.device(ResNet50(12, 7, False))
    with pytest.raises(ValueError, match="has not run a forward"):
        model.pooled()
    fc_weight, fc_bias, logit_weight, logit_bias = head_of(model)
    assert fc_weight.shape == (12, 2048) and logit_weight.shape == (7, 12) and logit_bias is None
    ops = NL.ops()
    batches = [(torch.rand(2, 3, 64, 64), torch.tensor([0, 3])), (torch.rand(2, 3, 64, 64), torch.tensor([-1, 6]))]
    for training in (False, True):
        model.train(training)
        with torch.no_grad():
            logits, features = model(tools.device(batches[0][0]))
        pooled = model.pooled()
        assert pooled.shape == (2, 2048) and pooled.dtype == torch.float32 and pooled.is_cuda
        assert bool(torch.isfinite(pooled).all()) and bool((pooled >= 0).all()) and float(pooled.max()) > 0
        again = ops.linear_fwd(pooled, fc_weight, fc_bias)
        assert torch.equal(again, features)
        assert torch.equal(ops.linear_fwd(again, logit_weight, None), logits)
        assert torch.equal(model.pooled(), pooled)
    default = get_arrays(model, batches)
    five = get_arrays(model, batches, pooled=True)
    assert len(default) == 4 and len(five) == 5 and five[4].shape == (4, 2048) and five[4].dtype == np.float32
    for a, b in zip(default, five):
        assert np.array_equal(a, b)
    assert np.array_equal(ops.linear_fwd(torch.from_numpy(five[4]).to(cuda), fc_weight, fc_bias).cpu().numpy(), five[2])


# ------------------------------------------------------------------------------------------------------------ end to end
P, F, C, N_TRAIN, M = 96, 12, 7, 300, 65
PERCENTILE = 70.0


def e2e_data():
    rng = np.random.default_rng(11)
    head = (rng.standard_normal((F, P)).astype(np.float32) * 0.2, rng.standard_normal(F).astype(np.float32),
            rng.standard_normal((C, F)).astype(np.float32), rng.standard_normal(C).astype(np.float32))
    train = np.maximum(rng.standard_normal((N_TRAIN, P)), 0).astype(np.float32)
    gt = rng.integers(0, C, N_TRAIN)
    gt[::9] = -1
    gt[4::31] = -2
    test = np.maximum(rng.standard_normal((M, P)) + 0.3, 0).astype(np.float32)
    test[3] = test[2]                                       # equal rows give equal scores
    return head, train, gt, test


@pytest.mark.parametrize("method", ("react", "ash_p", "ash_b", "ash_s", "scale"))
def test_end_to_end(cuda, method):
    from openset_imagenet import _native as NL
    from openset_imagenet.shaping import ActivationShaping
    head, train, gt, test = e2e_data()
    if method == "ash_b":
        head = head[:3] + (None,)                           # a head without a logit bias, as the evaluation network's
    ops = NL.ops()
    s = ActivationShaping(method, PERCENTILE).fit(train, gt, head=tuple(None if t is None else torch.from_numpy(t) for t in head))
    keep = 0
    if method == "react":
        counted = train[gt >= 0]
        assert s.count == len(counted) == int((gt >= 0).sum())
        want = np.percentile(counted.astype(np.float64), PERCENTILE)
        assert O.ulps(np.float32(s.clip), np.float32(want)) <= 1 and s.clip == O.linear_percentile(counted, PERCENTILE)[0]
        every = ActivationShaping(method, PERCENTILE).fit(train, head=head)
        assert every.count == N_TRAIN and O.ulps(np.float32(every.clip), np.float32(np.percentile(train.astype(np.float64), PERCENTILE))) <= 1
    else:
        keep = s.keep(P)
        assert s.clip is None and s.count is None and keep == P - 67
    shaped = s.shape(test)
    assert shaped.shape == (M, P) and shaped.is_cuda
    want, mask = O.shape_rows(test, O.MODES[method], keep, 0.0 if s.clip is None else s.clip)
    got = shaped.cpu().numpy()
    if method in ("react", "ash_p"):
        assert same_bits_nan(got, want)
    elif method == "ash_b":
        assert np.array_equal(got != 0, mask) and O.ulps(got, want).max() <= 1
    else:
        assert O.ulps(got, want).max() <= 2
    logits = s.logits(test)
    assert logits.shape == (M, C)
    by_hand = ops.linear_fwd(ops.linear_fwd(shaped, s.fc_weight, s.fc_bias), s.logit_weight, s.logit_bias)
    assert torch.equal(logits, by_hand)
    assert np.allclose(logits.cpu().numpy(), O.head(got, *head), rtol=0, atol=1e-3 * float(np.abs(O.head(got, *head)).max()))
    unknown = s.unknown_score(test)
    assert unknown.shape == (M,) and torch.equal(unknown, -ops.logit_scores(logits, NL.SCORE_ENERGY))
    assert torch.equal(s.energy(test), -unknown) and unknown[2] == unknown[3]
    lg = logits.cpu().numpy()
    for fn, mode in ((s.energy, O.ENERGY), (s.max_logit, O.MAXLOGIT), (s.msp, O.MSP)):
        assert O.ulps(fn(test).cpu().numpy(), O.logit_scores(lg, mode).astype(np.float32)).max() <= 1
    probs = s.predict(test)
    assert probs.shape == (M, C) and torch.equal(probs, ops.softmax(logits))
    assert np.abs(probs.cpu().numpy().astype(np.float64).sum(axis=1) - 1.0).max() <= C * 2.0 ** -23
    for fn in (s.shape, s.logits, s.predict, s.unknown_score, s.msp):
        assert torch.equal(fn(test, chunk=7), fn(test))
    loaded = ActivationShaping("scale", 33).load_state_dict(s.state_dict())
    assert loaded.fc_weight.device.type == "cpu" and (loaded.method, loaded.percentile, loaded.clip, loaded.count) == (
        method, PERCENTILE, s.clip, s.count)
    assert torch.equal(loaded.unknown_score(test), unknown) and torch.equal(loaded.predict(torch.from_numpy(test).to(cuda)), probs)
    assert s.shape(test[:0]).shape == (0, P) and s.unknown_score(test[:0]).shape == (0,)


# ------------------------------------------------------------------------------------------------------------ evaluate.py
def test_evaluate_main_writes_the_shaping_arrays_and_leaves_the_others_alone(cuda, tmp_path):
    """script/evaluate.py end to end on four JPEGs a split: `--shaping` adds its files, the arrays of the plain run and of another
    detector stay what they are without it, and the saved detector, restored, gives the scores main() wrote."""
    from PIL import Image
    from openset_imagenet import ResNet50, tools
    from openset_imagenet.script import evaluate
    from openset_imagenet.shaping import ActivationShaping, head_of
    from openset_imagenet.train import _image_loader, get_arrays, load_checkpoint
    tools.set_device_gpu(0)
    rng = np.random.default_rng(0)
    img_dir, proto, out = tmp_path / "imgs", tmp_path / "protocols", tmp_path / "out"
    for d in (img_dir, proto, out):
        d.mkdir()
    labels = {"train": (0, 1, 2, -1), "val": (0, 1, 2, -1), "test": (2, -2, 0, 1)}
    for split, ys in labels.items():
        for i, y in enumerate(ys):
            Image.fromarray(rng.integers(0, 256, size=(256, 256, 3), dtype=np.uint8)).save(img_dir / f"{split}_{i}.jpg", quality=90)
        (proto / f"p2_{split}.csv").write_text("".join(f"{split}_{i}.jpg,{y}\n" for i, y in enumerate(ys)))
    torch.manual_seed(3)
    torch.save({"epoch": 1, "model_state_dict": ResNet50(3, 3, False).state_dict(), "opt_state_dict": {}, "best_score": 0.5},
               out / "softmax_curr.pth")
    base = ["softmax", "2", "-g", "0", "--imagenet-directory", str(img_dir), "--protocol-directory", str(proto), "--output-directory",
            str(out), "--batch-size", "4", "--workers", "0"]
    plain = {k: dict(np.load(v)) for k, v in evaluate.main(base + ["--knn", "1"]).items()}
    assert sorted(plain) == ["test", "test_knn", "val", "val_knn"]
    more = {k: dict(np.load(v)) for k, v in evaluate.main(base + ["--knn", "1", "--shaping", "react", "--shaping-percentile", "80"]).items()}
    assert sorted(more) == ["test", "test_knn", "test_shaping", "val", "val_knn", "val_shaping"]
    for name, arrays in plain.items():                      # the same keys, dtypes and bits with the option on
        assert sorted(arrays) == sorted(more[name])
        for key, a in arrays.items():
            assert a.dtype == more[name][key].dtype and np.array_equal(a, more[name][key], equal_nan=True), (name, key)
    restored = ActivationShaping("scale").load_state_dict(torch.load(out / "softmax_shaping_curr.pth", weights_only=False))
    assert (restored.method, restored.percentile, restored.count) == ("react", 80.0, 3) and restored.clip > 0
    model = tools.device(ResNet50(3, 3, False))
    load_checkpoint(model, out / "softmax_curr.pth")
    for split in ("val", "test"):
        a = more[f"{split}_shaping"]
        assert sorted(a) == ["features", "gt", "logits", "scores", "unknown"] and a["scores"].shape == (4, 3) and a["unknown"].shape == (4,)
        for key in ("gt", "logits", "features"):
            assert np.array_equal(a[key], plain[split][key])
        ds = _image_loader(proto / f"p2_{split}.csv", img_dir, False, "eval")
        gt, logits, features, _, pooled = get_arrays(model, torch.utils.data.DataLoader(ds, batch_size=4, num_workers=0), pooled=True)
        assert np.array_equal(logits, a["logits"]) and pooled.shape == (4, 2048)
        back, again = evaluate.shaping_arrays(restored, dict(gt=gt, logits=logits, features=features, pooled=pooled), head_of(model), "react")
        assert back is restored and np.array_equal(again["scores"], a["scores"]) and np.array_equal(again["unknown"], a["unknown"])
        assert np.isfinite(a["unknown"]).all() and np.allclose(a["scores"].sum(axis=1), 1, atol=1e-5)
    fresh, scored = evaluate.shaping_arrays(dict(gt=gt, pooled=pooled), dict(gt=gt, logits=logits, features=features, pooled=pooled),
                                            head_of(model), "ash_s", 50)
    assert fresh.method == "ash_s" and fresh.keep(2048) == 1024 and scored["scores"].shape == (4, 3)

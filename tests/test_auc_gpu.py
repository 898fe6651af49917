"""GPU parity of the ROC-AUC mirror (metrics.auc_score_binary / auc_score_multiclass, csrc/auc.hip): the values the reference's own
functions returned (tests/golden/auc_reference.npz) within 1e-12, and the bits of the exact-count numpy oracle of
tests/test_auc_cpu.py everywhere: both sides form the same integers and the same one division."""
import struct

import numpy as np
import pytest
import torch

from test_auc_cpu import load_cases, mann_whitney, oracle_binary, oracle_multiclass, pair_counts

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def scores_with_ties(rng, N, C, dtype):
    """Softmax rows; every seventh row is cut down to multiples of 1/64 with the remainder added to its largest entry, so it still
    sums to 1 exactly (dyadic values) and ties with other such rows in every column."""
    z = rng.normal(size=(N, C)) * 3
    s = np.exp(z - z.max(1, keepdims=True)); s /= s.sum(1, keepdims=True)
    q = np.floor(s[::7] * 64) / 64
    q[np.arange(len(q)), q.argmax(1)] += 1.0 - q.sum(1)
    s[::7] = q
    return s.astype(dtype)


def labels_every_class(rng, N, C):
    gt = np.concatenate([np.arange(C), rng.integers(0, C, size=N - C)])
    rng.shuffle(gt)
    return gt.astype(np.int64)


def test_fixture_cases_host_and_device_inputs(cuda, golden_dir):
    from openset_imagenet.metrics import auc_score_binary, auc_score_multiclass
    for c in load_cases(golden_dir):
        gt, s = c["gt"], c["scores"]
        if c["kind"] == "binary":
            call = lambda y, x: auc_score_binary(y, x, unk_class=c["unk"])
            oracle = lambda: oracle_binary(gt, s, c["unk"])
        else:
            call = auc_score_multiclass
            oracle = lambda: oracle_multiclass(gt, s)
        for where in ("host", "device"):
            y, x = (gt.copy(), s.copy()) if where == "host" else (torch.from_numpy(gt).to(cuda), torch.from_numpy(s).to(cuda))
            if c["refused"]:
                with pytest.raises(ValueError):
                    call(y, x)
            else:
                got = call(y, x)
                assert isinstance(got, float)
                if np.isnan(c["auc"]):
                    assert np.isnan(got), (c["name"], where)
                else:
                    assert abs(got - c["auc"]) <= 1e-12, (c["name"], where, got, c["auc"])
                    assert same_bits(got, oracle()), (c["name"], where)
            # inputs are never written (the reference overwrites the labels with +-1)
            y2, x2 = (y, x) if where == "host" else (y.cpu().numpy(), x.cpu().numpy())
            assert np.array_equal(y2, gt) and np.array_equal(x2, s), (c["name"], where)


BINARY_EDGES = [(N, P) for N in (1, 2, 255, 256, 257, 513) for P in sorted({p for k in (0, 1, 256, 257) for p in (k, N - k) if 0 <= p <= N})]


def test_binary_tile_edges(cuda):
    """N around the 256-wide tiles with the positives or the negatives numbering 0, 1, 256 or 257; row widths that take one lane
    per row (C = 1), a partial lane group (C = 5) and more than one pass of a full wave (C = 70)."""
    from openset_imagenet.metrics import _auc_binary_counts, auc_score_binary
    rng = np.random.default_rng(7)
    for n, (N, P) in enumerate(BINARY_EDGES):
        C = (1, 5, 70)[n % 3]
        dtype = np.float64 if n % 4 == 3 else np.float32
        s = scores_with_ties(rng, N, C, dtype) if C > 1 else np.round(rng.random((N, 1)) * 16).astype(dtype) / 16
        gt = np.full(N, -1, dtype=np.int64)
        gt[rng.permutation(N)[:P]] = rng.integers(0, C, size=P)
        got, want = auc_score_binary(gt, s), oracle_binary(gt, s)
        assert (np.isnan(got) and np.isnan(want)) or same_bits(got, want), (N, P, C, got, want)
        m = s.max(1)
        assert _auc_binary_counts(gt, s, -1) == (*pair_counts(m[gt >= 0], m[gt < 0]), P, N - P, 0), (N, P, C)


@pytest.mark.parametrize("N,C,dtype", [(257, 3, np.float32), (513, 152, np.float32), (300, 1000, np.float32), (257, 30, np.float64)])
def test_ovr_tile_edges(cuda, N, C, dtype):
    """Per-class integers against the oracle's, then the value. At (300, 1000) most classes have no sample: the integers still have to
    agree class by class, and the public function refuses as sklearn does."""
    from openset_imagenet.metrics import _auc_ovr_counts, auc_score_multiclass
    rng = np.random.default_rng(N + C)
    s = scores_with_ties(rng, N, C, dtype)
    gt = labels_every_class(rng, N, C) if C <= N else rng.integers(0, C, size=N).astype(np.int64)
    g, e, pos, flags = _auc_ovr_counts(gt, s)
    assert flags == (0, 0, 0)
    want = [pair_counts(s[gt == c, c], s[gt != c, c]) for c in range(C)]
    assert pos == np.bincount(gt, minlength=C).tolist()
    assert list(zip(g, e)) == want
    assert sum(e) > 0                                          # the quantised rows do tie
    if C <= N:
        assert same_bits(auc_score_multiclass(gt, s), oracle_multiclass(gt, s))
    else:
        with pytest.raises(ValueError):
            auc_score_multiclass(gt, s)


def test_binary_counts_past_32_bits(cuda):
    from openset_imagenet.metrics import _auc_binary_counts, auc_score_binary
    N = 140000
    s = torch.full((N, 2), 0.5, dtype=torch.float32, device=cuda)
    gt = torch.zeros(N, dtype=torch.int64, device=cuda)
    gt[::2] = -1
    assert _auc_binary_counts(gt, s, -1) == (0, 4900000000, 70000, 70000, 0)
    assert auc_score_binary(gt, s) == 0.5


def test_protocol_sizes(cuda):
    from openset_imagenet.metrics import auc_score_binary, auc_score_multiclass
    rng = np.random.default_rng(20000)
    s = scores_with_ties(rng, 20000, 116, np.float32)
    gt = rng.integers(0, 116, size=20000); gt[rng.random(20000) < 0.4] = -1
    assert same_bits(auc_score_binary(gt, s), oracle_binary(gt, s))
    s = scores_with_ties(rng, 7001, 151, np.float32)
    gt = labels_every_class(rng, 7001, 151)
    assert same_bits(auc_score_multiclass(gt, s), oracle_multiclass(gt, s))


def test_refusals_and_casts(cuda):
    """NaN scores: ValueError from both, as sklearn. Scores of another dtype are cast to fp64 (here fp16: the comparisons then run on
    the fp16 values, exactly). A label outside 0..C-1 is refused by the multiclass form only."""
    from openset_imagenet.metrics import _auc_ovr_counts, auc_score_binary, auc_score_multiclass
    rng = np.random.default_rng(3)
    s = scores_with_ties(rng, 300, 9, np.float32)
    gt = labels_every_class(rng, 300, 9)
    bad = s.copy(); bad[123, 4] = np.nan
    for fn in (auc_score_binary, auc_score_multiclass):
        with pytest.raises(ValueError, match="NaN"):
            fn(gt, bad)
    assert _auc_ovr_counts(gt, bad)[3] == (0, 1, 1)            # the NaN row is also not a probability row
    known = np.where(gt < 3, -1, gt)
    s16 = s.astype(np.float16)
    assert same_bits(auc_score_binary(known, s16), oracle_binary(known, s16.astype(np.float64)))
    assert _auc_ovr_counts(known, s)[3] == (int((known < 0).sum()), 0, 0)
    with pytest.raises(ValueError, match="Number of classes"):
        auc_score_multiclass(known, s)


def test_evaluate_auc_row_selection(cuda):
    """`evaluate.py --auc`: for unk in {-1, -2} the known rows and the rows labelled unk only (rows of the other negative label would
    count as known), the background column dropped for the garbage loss; None when the split has no such row."""
    from openset_imagenet.metrics import auc_score_binary
    from openset_imagenet.script.evaluate import auc_rows
    rng = np.random.default_rng(11)
    N, C = 400, 6
    s = scores_with_ties(rng, N, C, np.float32)
    gt = rng.integers(0, C - 1, size=N).astype(np.float32)     # get_arrays() returns the labels as fp32
    r = rng.random(N); gt[r < 0.2] = -1; gt[r > 0.75] = -2
    for unk in (-1, -2):
        for loss in ("garbage", "entropic"):
            y, x = auc_rows(gt, s, unk, loss)
            keep = [i for i in range(N) if gt[i] >= 0 or gt[i] == unk]
            assert np.array_equal(y, gt[keep]) and np.array_equal(x, s[keep][:, :C - 1] if loss == "garbage" else s[keep])
            assert (y == unk).any() and not (y == (-3 - unk)).any()
            assert same_bits(auc_score_binary(y, x, unk_class=unk), oracle_binary(gt[keep], x, unk))
    assert auc_rows(np.where(gt == -2, -1, gt), s, -2, "entropic") is None

"""CPU: the float64 references and the case builders of tests/head_cases.py, checked without a kernel.

tests/test_head_kernels_gpu.py trusts three things that are shown here: the references are right (the oracle's restatement, taken on
rows selected by boolean-mask indexing, equals torch.nn.CrossEntropyLoss in value and gradient on every case the GPU file uses), every
label batch contains the kinds of row its case claims, and the planted rows do what the GPU test needs them for."""
import pytest
import torch
import torch.nn.functional as F

import head_cases as H
from oracle import losses_oracle as LO

EXACT = 1e-12       # two float64 evaluations of one expression: a few ulp of O(1..100) numbers


def _oracle(mode, z, y, w=1.0, cw=None, ignore_index=-1):
    z64 = z.double().clone().requires_grad_(True)
    J = H.oracle_loss64(mode, z64, y, w, cw, ignore_index)
    J.backward()
    return J.detach(), z64.grad


def _same(a, b, what):
    (Ja, ga), (Jb, gb) = a, b
    if bool(torch.isnan(Ja)) or bool(torch.isnan(Jb)):
        assert bool(torch.isnan(Ja)) and bool(torch.isnan(Jb)), what
        return
    assert abs(float(Ja) - float(Jb)) <= EXACT * max(1.0, abs(float(Jb))), what
    assert float((ga - gb).abs().max()) <= EXACT * max(1.0, float(gb.abs().max())), what


def _check_claims(mode, y, C, claims, ignore_index=-1):
    known, unknown, ignored = H.row_kinds(mode, y, C, ignore_index)
    assert int(known.sum()) >= claims["known"] and int(unknown.sum()) >= claims["unknown"] and int(ignored.sum()) >= claims["ignored"]
    assert bool((known.int() + unknown.int() + ignored.int() == 1).all()), "every row is of exactly one kind"


@pytest.mark.parametrize("case", H.LOSS_SHAPES, ids=H.loss_id)
@pytest.mark.parametrize("mode", list(H.MODES))
def test_loss_references_agree(mode, case):
    m = H.MODES[mode]
    B, C, scale, kind = case
    z, y, cw, claims = H.loss_case(m, case)
    assert z.shape == (B, C) and y.shape == (B,) and y.dtype == torch.int64
    _check_claims(m, y, C, claims)
    if B >= 15:     # the mixed batches hold every kind of row their mode has; the last-row case exactly one known row, the last
        known, unknown, ignored = H.row_kinds(m, y, C)
        if kind == "last_row_known":
            assert int(known.sum()) == 1 and bool(known[B - 1]) and (B - 1) % H.LOSS_WAVES != 0
        else:
            assert bool(known.any())
            assert bool((y == -1).any()) and (m != H.ENTROPIC or bool((y == -2).any())) and (m != H.GARBAGE or bool((y == -100).any()))
    masked = H.needs_mask(m, y, C)
    assert masked == (m == H.GARBAGE and bool((y == -1).any()))
    _same(_oracle(m, z, y, 1.0, cw), H.loss_ref64(m, z, y, 1.0, cw, -1, masked=masked), f"{mode} oracle vs CrossEntropyLoss")
    if not masked:  # boolean-mask indexing == what torch does with the whole batch
        _same(H.loss_ref64(m, z, y, 1.0, cw, -1, masked=True), H.loss_ref64(m, z, y, 1.0, cw, -1, masked=False), f"{mode} masked vs whole")
    if m == H.GARBAGE and cw.numel() > 1:
        assert bool((cw == 0).any()) and bool((cw > 0).any())
    n = H.normaliser(m, y, C, cw)
    if m == H.SOFTMAX:
        assert n == float(((y >= 0) & (y < C)).sum())
    if m == H.ENTROPIC:
        assert n == B


def test_entropic_unknown_weight_reference():
    z, y, _, _ = H.loss_case(H.ENTROPIC, (40, 65, 3.0, "mixed"))
    for w in (0.5, 2.0):
        _same(_oracle(H.ENTROPIC, z, y, w), H.loss_ref64(H.ENTROPIC, z, y, w), f"w = {w}")


def test_softmax_ignore_index_references_agree():
    seen = set()
    for name, z, y, ii, claims in H.softmax_ignore_cases():
        C = z.shape[1]
        _check_claims(H.SOFTMAX, y, C, claims, ii)
        assert bool((y == ii).any()), f"{name}: holds ignored rows"
        assert ii < 0 or bool(((y >= 0) & (y < C)).all()), "class-index ignore_index: torch takes class indices only"
        ref = H.loss_ref64(H.SOFTMAX, z, y, ignore_index=ii)
        _same(_oracle(H.SOFTMAX, z, y, ignore_index=ii), ref, name)
        if claims["known"] == 0:
            assert bool(torch.isnan(ref[0])), f"{name}: torch gives NaN"
        else:
            _same(H.loss_ref64(H.SOFTMAX, z, y, ignore_index=ii, masked=True), ref, name)
            assert float(ref[1][y == ii].abs().sum()) == 0
        seen.add(ii if ii <= 0 else "last")
    assert seen == {-1, 0, "last"}


def test_garbage_references_agree():
    names = []
    for name, z, y, cw, claims in H.garbage_cases():
        C = z.shape[1]
        _check_claims(H.GARBAGE, y, C, claims)
        assert bool((y == -100).any()) and not H.needs_mask(H.GARBAGE, y, C)
        ref = H.loss_ref64(H.GARBAGE, z, y, cw=cw)
        _same(_oracle(H.GARBAGE, z, y, cw=cw), ref, name)
        _same(H.loss_ref64(H.GARBAGE, z, y, cw=cw, masked=True), ref, name)
        used = cw[y[y >= 0]]
        if "present-classes" in name:
            assert float(used.sum()) == 0 and bool(torch.isnan(ref[0])), "total weight 0: torch gives NaN"
        elif "zero-weights" in name:
            assert bool((used == 0).any()) and bool((used > 0).any())
            assert float(ref[1][(y >= 0) & (cw[y.clamp(min=0)] == 0)].abs().sum()) == 0
        else:
            assert bool((cw > 0).all())
        assert float(ref[1][y == -100].nan_to_num().abs().sum()) == 0
        names.append(name)
    assert len(names) == 3


@pytest.mark.parametrize("B,C", [(17, 65), (40, 130)])
@pytest.mark.parametrize("mode", list(H.MODES))
def test_label_past_the_last_class_reference(mode, B, C):
    """The y >= C reference (that row's term removed, the mode's divisor kept) equals autograd of the oracle's expression; in
    entropic mode also the closed form (s_i p - t_i) / B with an all-zero row."""
    m = H.MODES[mode]
    z, y, cw, _ = H.loss_case(m, (B, C, 3.0, "mixed"))
    y, rows = H.with_labels_past_the_end(y, C)
    assert bool((y[rows] >= C).all()) and rows[0] < H.LOSS_WAVES and (B <= 19 or rows[-1] >= H.LOSS_WAVES)
    assert H.needs_mask(m, y, C) and bool(H.row_kinds(m, y, C)[2][rows].all())
    ref = H.loss_ref64(m, z, y, 1.0, cw, -1, masked=True)
    _same(_oracle(m, z, y, 1.0, cw), ref, mode)
    assert float(ref[1][rows].abs().sum()) == 0
    if m == H.ENTROPIC:
        closed = H.entropic_closed_form64(z, y, 1.0)
        assert float((closed - ref[1]).abs().max()) <= EXACT and float(closed[rows].abs().sum()) == 0
        # the divisor stays B: the loss is the full batch's sum without the removed rows' terms, over B
        keep = y < C
        full = torch.nn.CrossEntropyLoss(reduction="none")(z.double(), LO.entropic_targets(torch.where(keep, y, 0), C, 1.0, torch.float64))
        assert abs(float(full[keep].sum() / B) - float(ref[0])) <= EXACT * max(1.0, float(ref[0]))


def test_objectosphere_cases_hold_their_rows():
    assert all(Fd != C for _, C, Fd in H.OBJECTO_SHAPES)
    assert {B for B, _, _ in H.OBJECTO_SHAPES} == {16, 17, 40} and {Fd for _, _, Fd in H.OBJECTO_SHAPES} == {5, 64, 130}
    assert any(Fd < C for _, C, Fd in H.OBJECTO_SHAPES) and any(Fd > C for _, C, Fd in H.OBJECTO_SHAPES)
    for B, C, Fd in H.OBJECTO_SHAPES:
        for xi, alpha, w in H.OBJECTO_PARAMS:
            z, y, f = H.objecto_case(B, C, Fd, xi, H.gen(21, B, C, Fd))
            J, dz, df = H.objecto_ref64(z, y, f, w, xi, alpha)
            nrm = f.double().norm(dim=1)
            bases = (0,) if B <= 16 else (0, B - 4)
            assert B <= 16 or B - 4 + H.ROW_UNKNOWN >= H.LOSS_WAVES, "the second set of planted rows lies in a later trip"
            for base in bases:
                r = base + H.ROW_ZERO
                assert float(nrm[r]) == 0 and float(torch.nan_to_num(df[r]).abs().max()) == 0
                r = base + H.ROW_OUTSIDE
                assert int(y[r]) >= 0 and float(nrm[r]) > xi and float(df[r].abs().max()) == 0
                r = base + H.ROW_INSIDE
                assert int(y[r]) >= 0 and 0 < float(nrm[r]) < xi and float(df[r].abs().max()) > 0
                r = base + H.ROW_UNKNOWN
                assert int(y[r]) < 0 and float(nrm[r]) > 0 and float(df[r].abs().max()) > 0
            # the stated formula, written out with boolean masks
            known = y >= 0
            res = torch.cat([(xi - nrm[known]).clamp(min=0), nrm[~known]])
            want = H.loss_ref64(H.ENTROPIC, z, y, w)[0] + alpha * (res ** 2).sum() / B
            assert abs(float(J) - float(want)) <= EXACT * max(1.0, abs(float(want)))
            assert float((dz - H.loss_ref64(H.ENTROPIC, z, y, w)[1]).abs().max()) <= EXACT


def _confidence_by_masks(scores, y, offset, unknown_class, n_valid):
    unknown = y == unknown_class
    known = ~unknown & (y >= 0)
    rows = torch.arange(y.shape[0])
    kn = torch.stack([scores[i, y[i]] for i in rows[known]]).sum() / int(known.sum())
    ng = torch.stack([1.0 + offset - scores[i, :n_valid].max() for i in rows[unknown]]).sum() / int(unknown.sum())
    return float(kn), int(known.sum()), float(ng), int(unknown.sum())


@pytest.mark.parametrize("B,C", H.CONF_SHAPES)
def test_confidence_reference_and_cases(B, C):
    assert C > 64 and B > H.LOSS_WAVES
    for unknown_class in (-1, C - 1):
        scores, y = H.conf_case(B, C, unknown_class, H.gen(31, B, C, unknown_class + 1))
        assert scores.dtype == torch.float32 and float(scores.min()) > 0, "log(scores) is finite"
        s64 = scores.double()
        unknown = y == unknown_class
        known = ~unknown & (y >= 0)
        assert bool(known.any()) and bool(unknown.any()) and bool((y == -2).any())
        assert bool(unknown[H.LOSS_WAVES:].any()) and (B == H.LOSS_WAVES + 1 or bool(known[H.LOSS_WAVES:].any())), "rows of a later trip"
        results = {}
        for last in H.conf_last_valid(C):
            n_valid = C if last is None else (C + last if last < 0 else last)
            got = LO.confidence(s64, y, 1.0 / C, unknown_class, last)
            want = _confidence_by_masks(s64, y, 1.0 / C, unknown_class, n_valid)
            assert got[1] == want[1] and got[3] == want[3] and got[1] + got[3] + int((y == -2).sum()) <= B
            assert abs(got[0] - want[0]) <= EXACT and abs(got[2] - want[2]) <= EXACT
            results[n_valid] = got[2]
            # an off-by-one cut (one column more or one column fewer) changes the unknown side by far more than the 1e-6 of the GPU test
            if n_valid < C:
                wider = _confidence_by_masks(s64, y, 1.0 / C, unknown_class, n_valid + 1)
                assert abs(wider[2] - got[2]) > 1e-3
        assert len({round(v, 9) for v in results.values()}) == len(results), "every distinct cut gives its own value"


def test_softmax_cases():
    assert H.SOFTMAX_SHAPES == [(1, 1), (5, 64), (6, 65), (37, 151), (9, 1000)]
    for B, C in H.SOFTMAX_SHAPES:
        z = H.softmax_case(B, C, H.gen(41, B, C))
        ref = torch.softmax(z.double(), 1)
        assert not bool(torch.isnan(ref).any()) and float((ref.sum(1) - 1).abs().max()) <= 1e-12
        if B >= 3:
            assert float(z[0].max()) == 80 and float(z[0].min()) == -80
            assert bool(torch.isinf(z[1, ::3]).all()) and bool(torch.isfinite(z[1, 1::3]).all()) and float(ref[1, ::3].abs().max()) == 0
            assert float(z[2].max()) == float(z[2].min()) and float((ref[2] - 1.0 / C).abs().max()) <= 1e-15


def test_linear_reference_is_the_definition():
    for B, K, O in H.LINEAR_SHAPES:
        x, w, b, dy = H.linear_case(B, K, O, H.gen(51, B, K, O))
        y, dx, dw, db = H.linear_ref(x, w, b, dy, torch.float64)
        x64, w64, dy64 = x.double(), w.double(), dy.double()
        for got, want in ((y, x64 @ w64.t() + b.double()), (dx, dy64 @ w64), (dw, dy64.t() @ x64), (db, dy64.sum(0))):
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        assert H.linear_ref(x, w, None, dy, torch.float64)[3] is None
    assert any(K % 4 == 0 and K % 256 != 0 and K > 4 for _, K, _ in H.LINEAR_SHAPES), "f32x4 loop with a partial last stride"


def test_pooling_cases():
    for B, C, Hh, W in H.MAXPOOL_SHAPES:
        for kind in H.MAXPOOL_INPUTS:
            x, dy = H.maxpool_case(B, C, Hh, W, kind, H.gen(61, B, C, Hh, W, len(kind)))
            y64, dx64 = H.maxpool_ref(x, dy)
            assert dy.shape == y64.shape and torch.equal(dy * 64, (dy * 64).round()) and float(dy.abs().max()) <= 4
            # exact in fp32: the fp32 autograd result equals the float64 one bit for bit
            assert torch.equal(H.maxpool_ref(x, dy, torch.float32)[1].double(), dx64)
            assert abs(float(dx64.sum()) - float(dy.double().sum())) == 0, "every output gradient lands on exactly one input"
            if kind == "negative":
                assert float(x.max()) <= -1 and float(y64.max()) <= -1
                assert not torch.equal(F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2, 0), y64.float()), "zero padding would differ"
            if kind == "randn":
                assert float(y64.min()) < 0
            if kind == "relu" and x.numel() > 64:
                assert int((y64 == 0).sum()) > 0, "windows whose maximum is a tie at 0"
    assert any(Hh != W for _, _, Hh, W in H.MAXPOOL_SHAPES) and any(C < 8 for _, C, _, _ in H.MAXPOOL_SHAPES)
    assert {HW for _, HW, _ in H.AVGPOOL_SHAPES} == {1, 4, 9, 16, 50} and {C for _, _, C in H.AVGPOOL_SHAPES} == {4, 2048}
    for B, HW, C in H.AVGPOOL_SHAPES:
        x, dy = H.avgpool_case(B, HW, C, H.gen(71, HW, C))
        y64, dx64 = H.avgpool_ref64(x, dy)
        want = torch.flatten(F.adaptive_avg_pool2d(x.double().permute(0, 2, 1).reshape(B, C, HW, 1), 1), 1)
        assert float((y64 - want).abs().max()) <= 1e-14
        assert float((dx64 - (dy.double() / HW).unsqueeze(1).expand(B, HW, C)).abs().max()) <= 1e-15

"""The cases of tests/nonfinite_cases.py without a kernel: every reference gives the same non-finite mask in fp32 and fp64 (no GPU case
rests on a precision accident), contaminates what its case claims (no GPU case passes vacuously), and no case puts a non-finite
value against a structural zero. Plus the torch facts the contract of include/osi.h (non-finite values) rests on."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite_cases as NF

NAN, INF = NF.NAN, NF.INF


def _both(ref, *a):
    r32, r64 = ref(*a, torch.float32), ref(*a, torch.float64)
    for k in r64:
        if r64[k].is_floating_point():
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64, k
            assert NF.masks_equal(r32[k], r64[k]), f"{k}: fp32 and fp64 disagree on the non-finite set"            # (i)
    return r64


def _claim(expect, tensors, what=""):
    bad = [NF.nonfinite(t) for t in tensors]
    n_bad, n = sum(int(b.sum()) for b in bad), sum(b.numel() for b in bad)
    if expect == "partial":                                                                                      # (ii)
        assert 0 < n_bad < n, f"{what}: {n_bad} of {n} non-finite, the case claims partial contamination"
    elif expect == "none":                                                                                       # (iii)
        assert n_bad == 0, f"{what}: {n_bad} non-finite elements, the case claims none"
    else:
        assert n_bad == n, f"{what}: {n_bad} of {n} non-finite, the case claims all"


@pytest.mark.parametrize("case", NF.BN_CASES, ids=NF.bn_id)
def test_batchnorm_cases(case):
    d = NF.bn_inputs(case)
    r = _both(NF.bn_ref, case, d)
    names = NF.BN_FWD_OUTPUTS if case.operand == "y" else NF.BN_BWD_OUTPUTS
    for k in names:
        own, rest = NF.channel_of(k, r[k], NF.BN_C0)
        assert bool(torch.isfinite(rest).all()), f"{k}: another channel is contaminated"
        if case.expect == "none":
            assert bool(torch.isfinite(own).all()), k
        elif k != "gm":
            assert bool(NF.nonfinite(own).all()), f"{k}: channel {NF.BN_C0} is not non-finite throughout"
    if case.operand == "dout":
        assert bool(torch.isfinite(r["out"]).all()), "the backward cases run on a clean forward"
        assert abs(d["pre_at"]) > 0.1 and (d["pre_at"] > 0) == (case.gate == "open")
        assert int(NF.nonfinite(r["gm"]).sum()) == (1 if case.expect == "partial" else 0)
        assert d["at"][0] * case.H * case.H + d["at"][2] * case.H + d["at"][3] >= min(64, case.B * case.H * case.H // 2)


@pytest.mark.parametrize("case", NF.BNSTATS_CASES, ids=lambda c: f"H{c.H}")
def test_conv_statistics_cases(case):
    r = _both(NF.bnstats_ref, case, NF.bnstats_inputs(case))
    _claim(case.expect, list(r.values()))


def _no_structural_zero(case, d, H, W):
    if case.operand == "w":                                                                                      # (iv)
        assert case.op == "fwd" and bool(torch.isnan(d["w"][NF.CONV_K0]).all()) and bool(torch.isfinite(d["w"][:NF.CONV_K0]).all())
    if case.op == "wgrad" and case.operand == "dy" and d["pad"] > 0:
        assert NF.conv_taps_inside(d, H, W), "a poisoned dy of a padded weight gradient must see all its taps inside the image"
    if case.op == "wgrad" and case.operand == "x" and d["pad"] > 0:      # ... and a poisoned x no output pixel outside it
        _, _, h, w = d["at"]
        assert case.where == "interior" and d["k"] - 1 <= h < H - d["k"] + 1 and d["k"] - 1 <= w < W - d["k"] + 1


@pytest.mark.parametrize("case", NF.CONV_CASES + [NF.SPLITK_CASE], ids=NF.conv_id)
def test_convolution_cases(case):
    d = NF.conv_inputs(case)
    _no_structural_zero(case, d, case.H, case.H)
    r = _both(NF.conv_ref, case, d)
    _claim(case.expect, list(r.values()), NF.conv_id(case))
    if case.op == "wgrad" and case.operand == "dy":
        bad = NF.nonfinite(r["dw"])
        assert bool(bad[NF.CONV_K0].all()) and int(bad.sum()) == bad[NF.CONV_K0].numel(), "exactly the filters of that output channel"


@pytest.mark.parametrize("case", NF.WINO_CASES, ids=NF.conv_id)
def test_winograd_cases(case):
    d = NF.conv_inputs(case, case.W)
    _no_structural_zero(case, d, case.H, case.W)
    r = _both(NF.conv_ref, case, d)
    _claim(case.expect, list(r.values()), NF.conv_id(case))


@pytest.mark.parametrize("case", NF.ACT_CASES, ids=NF.act_id)
def test_fused_activation_cases(case):
    d = NF.act_inputs(case)
    r = _both(NF.act_ref, case, d)
    _claim(case.expect, list(r.values()), NF.act_id(case))
    if case.entry.startswith("wgrad"):
        bad = NF.nonfinite(r["dw"])
        assert int(bad.sum()) == int(bad[..., NF.ACT_C0].sum()) > 0, "only the weight gradient towards that input channel"
        if case.stride == 1 or case.operand == "shift":      # (a stride-2 layer reads one pixel through the taps of its parity class only)
            assert bool(bad[..., NF.ACT_C0].all())


@pytest.mark.parametrize("case", NF.EPI_CASES + NF.EPI_WINO_CASES, ids=NF.epi_id)
def test_inference_epilogue_cases(case):
    clean, bad = NF.epi_inputs(case)
    assert bool(torch.isfinite(NF.epi_ref(case, clean, torch.float64)["out"]).all())
    r = _both(NF.epi_ref, case, bad)
    _claim(case.expect, [r["out"]], NF.epi_id(case))
    m = NF.nonfinite(r["out"])
    if case.operand == "x":
        assert int(m.sum()) == int(m[NF.EPI_IMAGE].sum()) == case.Cout * case.k * case.k, "the receptive field of that pixel, in its image only"
    elif case.operand == "scale":
        assert bool(m[..., NF.EPI_N0].all()) and int(m.sum()) == m[..., NF.EPI_N0].numel()
    else:
        assert int(m.sum()) == 1


@pytest.mark.parametrize("case", NF.POOL_CASES, ids=NF.pool_id)
def test_pool_cases(case):
    d = NF.pool_inputs(case)
    r = _both(NF.pool_ref, case, d)
    _claim(case.expect, [r["y"]], NF.pool_id(case))
    if case.value == "nan":
        flat = r["act"].flatten(2)
        named = torch.gather(flat, 2, r["idx"].flatten(2)).view(r["y"].shape)
        assert bool(torch.isnan(named[torch.isnan(r["y"])]).all()), "torch's index names a NaN element"
        for b, c, h, w in d["at"]:      # every window that holds the element
            assert bool(torch.isnan(r["y"][b, c, h // 2:(h + 1) // 2 + 1, w // 2:(w + 1) // 2 + 1]).all())
    if case.value == "+inf":
        assert int((r["y"] == INF).sum()) == int(NF.nonfinite(r["y"]).sum()), "+Inf wins its windows"


@pytest.mark.parametrize("which", ["avgpool", "linear"])
def test_avgpool_and_linear_cases(which):
    r = _both(NF.avgpool_linear_ref, which, NF.avgpool_linear_inputs(which))
    _claim("partial", [v for v in r.values()], which)


@pytest.mark.parametrize("case", NF.LOSS_CASES, ids=NF.loss_id)
def test_loss_cases(case):
    import head_cases as H
    d = NF.loss_inputs(case)
    known, unknown, ignored = H.row_kinds(d["mode"], d["y"], NF.LOSS_C)
    assert bool((known | unknown)[d["row"]]) == (case.row == "counted")
    r = _both(NF.loss_ref, case, d)
    assert bool(torch.isfinite(r["loss"])) == (case.row != "counted"), "only a counted row reaches the loss"
    _claim(case.expect, [r["dz"]], NF.loss_id(case))
    bad = NF.nonfinite(r["dz"])
    assert int(bad.sum()) == int(bad[d["row"]].sum()), "only the poisoned row's gradient is touched"


@pytest.mark.parametrize("row", NF.OBJECTO_ROWS)
def test_objectosphere_cases(row):
    d = NF.objecto_inputs(row)
    r32, r64 = NF.objecto_ref(d, torch.float32), NF.objecto_ref(d, torch.float64)
    for k in r64:
        assert NF.masks_equal(r32[k], r64[k]), k
    assert bool(torch.isnan(r64["loss"])) and bool(torch.isfinite(r64["dz"]).all())
    bad = NF.nonfinite(r64["df"])
    assert bool(bad[d["row"]].all()) and int(bad.sum()) == NF.OBJECTO_F, "the whole feature-gradient row, and only it"


def test_softmax_and_confidence_cases():
    z = NF.softmax_inputs()
    s32, s64 = torch.softmax(z, 1), torch.softmax(z.double(), 1)
    assert NF.masks_equal(s32, s64) and bool(NF.nonfinite(s64)[3:5].all()) and int(NF.nonfinite(s64).sum()) == 2 * z.shape[1]
    from oracle import losses_oracle as LO
    for form in ("scores", "logits"):
        for kind, slot in (("known", 0), ("negative", 2)):
            arg, y, offset, unk, row = NF.conf_inputs(kind, form)
            a32, a64 = (NF.conf_ref(arg, y, offset, unk, form, dt) for dt in (torch.float32, torch.float64))
            assert NF.masks_equal(a32, a64) and bool(torch.isnan(a64[slot])) and bool(torch.isfinite(a64[2 - slot]))
            # the restatement is the oracle's: on the clean rows the two agree
            clean = torch.nan_to_num(arg if form == "scores" else torch.softmax(arg.double(), 1), nan=0.25).double()
            kn, kc, ng, nc = LO.confidence(clean, y, offset, unk, None)
            ref = NF.conf_ref(clean, y, offset, unk, "scores", torch.float64)
            assert (kc, nc) == (float(ref[1]), float(ref[3])) and abs(kn * kc - float(ref[0])) < 1e-9 and abs(ng * nc - float(ref[2])) < 1e-9


def test_whole_network_cases():
    """The oracle in training mode reports NaN logits and a NaN loss for both poisons; in eval mode only the poisoned image's row."""
    from oracle import resnet50_oracle as R, losses_oracle as L
    for poison in NF.NET_POISONS:
        sd, x, y, _ = NF.network_inputs(poison)
        with torch.no_grad():
            lg, _ = R.forward({k: v.clone() for k, v in sd.items()}, x, True)
        assert bool(torch.isnan(lg).all()) and bool(torch.isnan(L.entropic_openset_loss(lg, y, 1.0)))
    sd, x, _, clean = NF.network_inputs("pixel", image=2)
    with torch.no_grad():
        lg, ft = R.forward({k: v.clone() for k, v in sd.items()}, x, False)
        lg0, ft0 = R.forward({k: v.clone() for k, v in sd.items()}, clean, False)
    rows = [0, 1, 3]
    assert bool(torch.isnan(lg[2]).all()) and bool(torch.isnan(ft[2]).all())
    assert torch.equal(lg[rows], lg0[rows]) and torch.equal(ft[rows], ft0[rows])


# ---- the torch facts the contract rests on ---------------------------------------------------------------------------------------
def test_torch_relu_keeps_nan():
    assert bool(torch.isnan(F.relu(torch.tensor([NAN, -1.0, 2.0]))[0]))
    assert float(F.relu(torch.tensor(-INF))) == 0 and float(F.relu(torch.tensor(INF))) == INF


def test_torch_max_pool_returns_nan_and_names_it():
    x = torch.arange(25.0).view(1, 1, 5, 5)
    x[0, 0, 1, 1] = NAN                                   # rows / columns 1 belong to the windows 0 and 1
    y, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    assert bool(torch.isnan(y[0, 0, :2, :2]).all()) and int(torch.isnan(y).sum()) == 4
    assert bool((idx[0, 0, :2, :2] == 6).all())
    x[0, 0, 1, 2] = NAN                                   # two in the windows of column 1: torch names one of them (which: not asserted)
    y, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    assert set(idx[0, 0, :2, 1].tolist()) <= {6, 7} and bool(torch.isnan(y[0, 0, :2, :2]).all())


def test_torch_batch_norm_with_one_inf():
    x = torch.randn(4, 3, 5, 5, dtype=torch.float64)
    x[1, 1, 2, 2] = INF
    rm, rv = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    out = F.batch_norm(x, rm, rv, None, None, True, 0.1, 1e-5)
    assert float(rm[1]) == INF and bool(torch.isnan(rv[1])) and bool(torch.isnan(out[:, 1]).all())
    assert bool(torch.isfinite(out[:, [0, 2]]).all()) and bool(torch.isfinite(rm[[0, 2]]).all()) and bool(torch.isfinite(rv[[0, 2]]).all())
    assert float(x[:, 1].mean()) == INF and bool(torch.isnan(x[:, 1].var(unbiased=False)))


def test_torch_cross_entropy_ignores_a_nan_row():
    z = torch.randn(5, 7, dtype=torch.float64)
    z[2, 3] = NAN
    y = torch.tensor([0, 1, -1, 3, 4])
    zz = z.clone().requires_grad_(True)
    J = F.cross_entropy(zz, y, ignore_index=-1)
    J.backward()
    assert bool(torch.isfinite(J)) and bool(torch.isfinite(zz.grad[[0, 1, 3, 4]]).all())


def test_torch_max_of_a_row_with_nan_is_nan():
    s = torch.rand(3, 6)
    s[1, 4] = NAN
    m = torch.max(s, dim=1)[0]
    assert bool(torch.isnan(m[1])) and bool(torch.isfinite(m[[0, 2]]).all())

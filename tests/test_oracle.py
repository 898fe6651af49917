"""CPU: the oracle (oracle/*.py) against vectors produced by the reference's own files (tests/golden/losses_reference.npz,
written by tests/golden/make_golden.py from /root/reference/openset_imagenet/{losses,metrics,dataset}.py) and against the
structural anchors of the reference model (parameter counts, state_dict keys)."""
import os

import numpy as np
import pytest
import torch

from oracle import losses_oracle as L
from oracle import resnet50_oracle as R


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "losses_reference.npz"))


def _grad(fn, z):
    z = z.clone().requires_grad_(True)
    j = fn(z)
    j.backward()
    return j.detach(), z.grad


def test_entropic_loss_matches_reference(G):
    for name in G["eos.names"]:
        p = f"eos.{name}."
        z, y, w = torch.from_numpy(G[p + "logits"]), torch.from_numpy(G[p + "target"]), float(G[p + "w"])
        j, g = _grad(lambda t: L.entropic_openset_loss(t, y, w), z)
        assert abs(float(j) - float(G[p + "loss"])) <= 2e-6 * max(1, abs(float(G[p + "loss"]))), p
        assert np.allclose(g.numpy(), G[p + "dlogits"], atol=3e-7), p
        # closed form of SURVEY.md Appendix B.1: grad = (s_i p - t_i) / B
        t = L.entropic_targets(y, z.shape[1], w, torch.float64)
        closed = (t.sum(1, keepdim=True) * torch.softmax(z.double(), 1) - t) / z.shape[0]
        assert np.allclose(closed.numpy(), G[p + "dlogits"], atol=3e-7), p


def test_softmax_loss_matches_reference(G):
    for name in G["sm.names"]:
        p = f"sm.{name}."
        z, y = torch.from_numpy(G[p + "logits"]), torch.from_numpy(G[p + "target"])
        ref = float(G[p + "loss"])
        if np.isnan(ref):
            assert torch.isnan(L.softmax_loss(z, y)), "all-ignored batch -> NaN (torch semantics, kept)"
            continue
        j, g = _grad(lambda t: L.softmax_loss(t, y), z)
        assert abs(float(j) - ref) <= 2e-6 * max(1, abs(ref)), p
        assert np.allclose(g.numpy(), G[p + "dlogits"], atol=3e-7), p


def test_garbage_loss_and_class_weights_match_reference(G):
    for name in G["gb.names"]:
        p = f"gb.{name}."
        z, y = torch.from_numpy(G[p + "logits"]), torch.from_numpy(G[p + "target"])
        cw = L.class_weights(torch.from_numpy(G[p + "csv_labels"]))
        assert np.allclose(cw.numpy(), G[p + "class_weights"], rtol=1e-6), p
        j, g = _grad(lambda t: L.garbage_loss(t, y, cw), z)
        assert abs(float(j) - float(G[p + "loss"])) <= 2e-6 * max(1, abs(float(G[p + "loss"]))), p
        assert np.allclose(g.numpy(), G[p + "dlogits"], atol=3e-7), p
    # worked example of SURVEY.md Appendix B.5
    labels = torch.tensor([-1] * 3 + [0] * 4 + [1] * 5 + [2] * 6)
    assert np.allclose(L.class_weights(labels).numpy(), G["cw.example"])
    assert np.allclose(G["cw.example"], [1.125, 0.9, 0.75, 1.5])


def test_confidence_matches_reference(G):
    for name in G["conf.names"]:
        p = f"conf.{name}."
        off, unk, last = G[p + "args"]
        r = L.confidence(torch.from_numpy(G[p + "scores"]), torch.from_numpy(G[p + "target"]), float(off), int(unk),
                         None if last == -999 else int(last))
        assert np.allclose(np.array(r, dtype=np.float64), G[p + "result"], rtol=1e-6, atol=1e-7), p


def test_objectosphere_definition():
    """Build-defined term (parity unpinned): check the stated formula and its gradient on a hand-computable case."""
    z = torch.zeros(2, 4)
    y = torch.tensor([1, -1])
    f = torch.tensor([[3.0, 4.0, 0, 0], [0.0, 0.0, 2.0, 0]], requires_grad=True)
    j = L.objectosphere_loss(z, y, f, 1.0, xi=10.0, alpha=0.5)
    eos = float(L.entropic_openset_loss(z, y, 1.0))
    assert abs(float(j) - (eos + 0.5 * ((10 - 5) ** 2 + 2 ** 2) / 2)) < 1e-6
    j.backward()
    assert torch.allclose(f.grad[0], torch.tensor([-0.5 * 2 * 5 * 0.6 / 2, -0.5 * 2 * 5 * 0.8 / 2, 0, 0]))
    assert torch.allclose(f.grad[1], torch.tensor([0, 0, 0.5 * 2 * 2 / 2, 0.0]))


def test_model_structure_anchors():
    convs = R.conv_inventory()
    assert len(convs) == 53 and len({(c[1], c[2], c[3], c[4]) for c in convs}) <= 23
    conv_params = sum(cin * cout * k * k for _, cin, cout, k, _, _ in convs)
    bn_affine = sum(2 * cout for _, _, cout, *_ in convs)
    assert conv_params == 23454912 and bn_affine == 53120
    for C, total in ((30, 23570402), (116, 23759172), (152, 23842584), (1000, 26557032)):
        assert conv_params + bn_affine + 2048 * C + C + C * C == total
    keys = R.state_keys()
    assert len(keys) == 321 and keys[0] == "resnet_base.conv1.weight" and keys[-1] == "logits.weight"
    sd = R.init_state(10, 10)
    assert list(sd) == keys and len(R.param_keys(sd)) == 162
    macs = 0
    h = 224
    for name, cin, cout, k, s, pad in convs:
        hin = 224 if name.endswith("base.conv1") else None
    # MAC count at 224x224 = 4 087 136 256
    hw = {"stem": 224}
    x = 224
    total = 0
    x = (x + 6 - 7) // 2 + 1; total += x * x * 64 * 3 * 49
    x = (x + 2 - 3) // 2 + 1
    inpl = 64
    for planes, blocks, stride in R.STAGES:
        for b in range(blocks):
            st = stride if b == 0 else 1
            total += x * x * inpl * planes
            xo = (x + 2 - 3) // st + 1
            total += xo * xo * planes * planes * 9 + xo * xo * planes * planes * 4
            if b == 0:
                total += xo * xo * inpl * planes * 4
            x, inpl = xo, planes * 4
    assert total == 4087136256


def test_oracle_forward_reproduces_committed_vectors(golden_dir):
    """The oracle at the committed seeds reproduces tests/golden/model_oracle.npz (guards against silent drift of the restatement)."""
    V = np.load(os.path.join(golden_dir, "model_oracle.npz"))
    tag, (B, HW, C, seed) = "b8_128_c30", V["b8_128_c30.meta"]
    gen = torch.Generator().manual_seed(int(seed))
    sd = R.init_state(int(C), int(C), False, generator=gen)
    x = torch.rand(int(B), 3, int(HW), int(HW), generator=gen)
    logits, feats = R.forward({k: v.clone() for k, v in sd.items()}, x, True)
    assert np.allclose(logits.numpy(), V[f"{tag}.f32.logits"], atol=2e-5)
    assert np.allclose(logits.numpy(), V[f"{tag}.f64.logits"], atol=1e-4)


def test_oscr_oracle_matches_reference(golden_dir):
    """oracle/oscr_oracle.py (sort + binary search) against the vectors produced by the reference's own calculate_oscr loop
    (util.py:90-122; tests/golden/make_golden_oscr.py): identical float64 arrays, nan for an absent sample class included."""
    from oracle.oscr_oracle import calculate_oscr
    G = np.load(os.path.join(golden_dir, "oscr_reference.npz"))
    assert len(G["names"]) >= 10
    for n in G["names"]:
        ccr, fpr = calculate_oscr(G[f"{n}.gt"], G[f"{n}.scores"], int(G[f"{n}.unk"]))
        assert ccr.dtype == np.float64 and ccr.shape == G[f"{n}.ccr"].shape, n
        assert np.array_equal(ccr, G[f"{n}.ccr"], equal_nan=True), n
        assert np.array_equal(fpr, G[f"{n}.fpr"], equal_nan=True), n


def test_oracle_body_matches_transformers_witness(golden_dir):
    """The ResNet-50 body of the oracle against an INDEPENDENT implementation of the same published topology:
    transformers' ResNetModel configured as ResNet-50 v1.5 (tests/golden/make_golden_witness.py, run in the dev container;
    torchvision — the reference's own source of the body, model.py:17 — is not installed anywhere). The weights are
    regenerated here from the same seeds; only the witness OUTPUTS are stored. fp64 on both sides, train and eval mode,
    including the running-statistics update rule. Tolerance 1e-9 (pure summation-order noise in float64)."""
    W = np.load(os.path.join(golden_dir, "resnet_witness.npz"))
    assert len(W["names"]) >= 2
    for tag in W["names"]:
        B, HW, C, seed = (int(v) for v in W[f"{tag}.meta"])
        gen = torch.Generator().manual_seed(seed)
        sd = R.randomize_bn(R.init_state(C, C, False, generator=gen), gen)
        x = torch.rand(B, 3, HW, HW, generator=gen).double()
        for mode in ("train", "eval"):
            work = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
            taps = {}
            logits, feats = R.forward(work, x, mode == "train", taps)
            p = f"{tag}.{mode}."
            for name, got in (("pooled", taps["pooled"]), ("features", feats), ("logits", logits)):
                ref = W[p + name]
                assert got.shape == ref.shape, (p, name)
                assert float(np.abs(got.numpy() - ref).max()) <= 1e-9 * max(1.0, float(np.abs(ref).max())), (p, name)
            if mode == "train":
                for key in W.files:
                    if key.startswith(p + "resnet_base.") and key.endswith(("running_mean", "running_var")):
                        assert np.allclose(work[key[len(p):]].numpy(), W[key], rtol=1e-10, atol=1e-12), key
                        assert int(work[key[len(p):].rsplit(".", 1)[0] + ".num_batches_tracked"]) == 1
        # the float32 oracle (the one the HIP path is compared with) stays within its usual noise of the witness
        work = {k: v.clone() for k, v in sd.items()}
        lg32, _ = R.forward(work, x.float(), True)
        assert float(np.abs(lg32.double().numpy() - W[f"{tag}.train.logits"]).max()) <= 1e-4
        # backward: the witness's autograd gradients of the entropic loss (fp64) against the oracle's, all 162 norms + the committed
        # tensors / strided samples. Both sides are fp64 with the same decisions (no pre-activation sits within 1e-16 of zero), so
        # the bar is summation-order noise: 1e-8 relative.
        y = torch.from_numpy(W[f"{tag}.grad.labels"])
        work = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        _, _, loss, grads = R.forward_backward(work, x, y, lambda lg, t, f: L.entropic_openset_loss(lg, t, 1.0))
        assert abs(float(loss) - float(W[f"{tag}.grad.loss"])) <= 1e-12 * max(1.0, abs(float(loss)))
        keys = R.param_keys(sd)
        norms = np.array([float(grads[k].norm()) for k in keys])
        assert norms.shape == W[f"{tag}.grad.norms"].shape == (162,)
        assert np.allclose(norms, W[f"{tag}.grad.norms"], rtol=1e-8, atol=1e-14), tag
        checked = 0
        for key in W.files:
            if key.startswith(f"{tag}.grad.full."):
                k = key[len(f"{tag}.grad.full."):]
                got = grads[k].numpy()
            elif key.startswith(f"{tag}.grad.every"):
                n, k = key[len(f"{tag}.grad.every"):].split(".", 1)
                got = grads[k].flatten()[::int(n)].numpy()
            else:
                continue
            ref = W[key]
            assert got.shape == ref.shape, key
            assert float(np.abs(got - ref).max()) <= 1e-8 * float(np.abs(ref).max()) + 1e-16, key
            checked += 1
        assert checked >= 20


def test_host_classes_match_reference_traces(golden_dir, tmp_path):
    """AverageMeter / EarlyStopping (reference losses.py:32-94) and NameSpace / load_yaml (util.py:16-34) of the drop-in package against
    traces produced by executing the reference's own classes (tests/golden/make_golden_misc.py): same values after every update /
    call, same repr, same dict() and dump() of a loaded configuration."""
    import openset_imagenet as oi
    G = np.load(os.path.join(golden_dir, "misc_reference.npz"))
    m = oi.AverageMeter()
    for (v, c), ref in zip(G["am.updates"], G["am.trace"]):
        m.update(float(v), int(c))
        assert (m.val, m.avg, m.sum, m.count) == tuple(ref)
    assert repr(m) == str(G["am.repr"])
    m.reset()
    assert [m.val, m.avg, m.sum, m.count] == list(G["am.after_reset"])
    for tag in G["es.names"]:
        patience, delta, loss_mode = G[f"es.{tag}.args"]
        es = oi.EarlyStopping(patience=int(patience), delta=float(delta))
        for v, (counter, best, stop) in zip(G[f"es.{tag}.values"], G[f"es.{tag}.trace"]):
            es(float(v), loss=bool(loss_mode))
            assert (es.counter, es.best_score, float(es.early_stop)) == (counter, best, stop), tag
    y = tmp_path / "c.yaml"
    y.write_text(str(G["ns.yaml_text"]))
    cfg = oi.util.load_yaml(y)
    assert cfg.dump() == str(G["ns.dump"]) and repr(cfg.dict()) == str(G["ns.dict_repr"])
    assert cfg.loss.type == str(G["ns.loss_type"]) and cfg.opt.lr == float(G["ns.lr"]) and (cfg.gpu is None) == bool(G["ns.gpu_is_none"])
    assert cfg.dist.distributed is True and cfg.parallel is False and cfg.checkpoint is None


def test_gate_pinned_fp32_vs_fp64_anchor():
    """Anchor of the whole-network gradient bar (tests/test_gate_pinned_gpu.py): torch-CPU fp32 against the fp64 run, free-running
    and with the fp64 run's ReLU / arg-max decisions pinned. Free: ~1.4e-2 on every tensor (a few dozen flipped decisions out of
    1.3e7). Pinned: 4.7e-5 median / 1.3e-4 max — so a 5e-4 bar for an fp32 implementation under pinned decisions is a real bar.
    Also: pinning a run to its OWN decisions changes nothing, bit for bit (the hook is value-preserving)."""
    import numpy as np
    g = torch.Generator().manual_seed(5)
    B, HW, C = 8, 96, 30
    sd = R.init_state(C, C, False, generator=g)
    x = torch.rand(B, 3, HW, HW, generator=g)
    y = torch.randint(-1, C, (B,), generator=g)
    fn = lambda lg, t, f: L.entropic_openset_loss(lg, t, 1.0)
    sd64 = lambda: {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    rec64, rec32 = {}, {}
    r64 = R.forward_backward(sd64(), x.double(), y, fn, record_gates=rec64)
    r32 = R.forward_backward({k: v.clone() for k, v in sd.items()}, x, y, fn, record_gates=rec32)
    r32p = R.forward_backward({k: v.clone() for k, v in sd.items()}, x, y, fn, gates=rec64)
    r64p = R.forward_backward(sd64(), x.double(), y, fn, gates=rec64)
    rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
    free = [rel(r32[3][k], r64[3][k]) for k in r64[3]]
    pinned = [rel(r32p[3][k], r64[3][k]) for k in r64[3]]
    assert len(rec64["relu"]) == 49 and len(pinned) == 162
    assert torch.equal(r64p[0], r64[0]) and all(torch.equal(r64p[3][k], r64[3][k]) for k in r64[3])
    flips, pool_flips, total = R.gate_disagreements(rec32, rec64)
    print(f"free {np.median(free):.2e}/{max(free):.2e}  pinned {np.median(pinned):.2e}/{max(pinned):.2e}  flips {flips}/{total} pool {pool_flips}")
    assert 0 < flips <= 2e-5 * total and pool_flips <= 5
    assert np.median(free) > 3e-3                       # the free-running comparison is dominated by the flips ...
    assert np.median(pinned) <= 1e-4 and max(pinned) <= 3e-4   # ... and two orders tighter without them


def test_bn_states_reproduce_the_previous_draws_and_hold_every_class():
    """kind = "positive" of tests/osi_testlib.py::bn_state and of randomize_bn is the expression the tests used before the kind
    existed, number for number; kind = "signed" leaves the generator where "positive" leaves it, holds the seven classes of its table,
    and refuses a channel count that cannot hold them plus a dead channel."""
    import osi_testlib as T
    for beta_std in (1.0, 0.7, 0.3):
        g1, g2 = torch.Generator().manual_seed(17), torch.Generator().manual_seed(17)
        ga, be = T.bn_state(70, g1, "positive", beta_std)
        old_ga, old_be = torch.rand(70, generator=g2) + 0.5, torch.randn(70, generator=g2) * beta_std
        assert torch.equal(ga, old_ga) and torch.equal(be, old_be) and ga.dtype == torch.float32
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    sd = R.randomize_bn(R.init_state(4, 4, generator=g1), generator=g1)
    old = R.init_state(4, 4, generator=g2)
    for k in list(old):
        if k.endswith("running_mean"):
            pre, c = k[:-len("running_mean")], old[k].numel()
            old[pre + "weight"] = (0.5 + torch.rand(c, generator=g2)).to(old[k].dtype)
            old[pre + "bias"] = (0.2 * torch.randn(c, generator=g2)).to(old[k].dtype)
            old[pre + "running_mean"] = (0.1 * torch.randn(c, generator=g2)).to(old[k].dtype)
            old[pre + "running_var"] = (0.5 + torch.rand(c, generator=g2)).to(old[k].dtype)
    assert list(sd) == list(old) and all(torch.equal(sd[k], old[k]) for k in old)
    # signed: same generator consumption, the table's values, running statistics as for "positive"
    g3 = torch.Generator().manual_seed(3)
    sg = R.randomize_bn(R.init_state(4, 4, generator=g3), generator=g3, kind="signed")
    assert torch.equal(torch.rand(5, generator=g1), torch.rand(5, generator=g3))
    for k in sg:
        if k.endswith(("running_mean", "running_var")) or "bn" not in k and "downsample.1" not in k:
            assert torch.equal(sg[k], sd[k]), k
    ga, be = sg["resnet_base.layer1.0.bn3.weight"], sg["resnet_base.layer1.0.bn3.bias"]
    pos = sd["resnet_base.layer1.0.bn3.weight"]
    cls = torch.arange(256) % 7
    assert torch.equal(ga[cls == 0], pos[cls == 0]) and torch.equal(ga[(cls == 1) | (cls == 6)], -pos[(cls == 1) | (cls == 6)])
    assert float(be[cls <= 1].std()) > 0.4 and bool((ga[cls == 0] >= 0.5).all())
    for c, (gv, bv) in {2: (0.0, 0.7), 3: (0.0, 0.0), 4: (-0.05, 1.0), 5: (0.05, -1.0)}.items():
        assert bool((ga[cls == c] == gv).all()) and bool((be[cls == c] == torch.tensor(bv)).all())
    ga2, be2 = T.bn_state(256, torch.Generator().manual_seed(9), "signed")
    assert torch.equal(ga2 == 0, (cls == 2) | (cls == 3)) and bool(((ga2 < 0) == ((cls == 1) | (cls == 4) | (cls == 6))).all())
    assert int(T.dead_channels(12).sum()) == 1 and set(T.bn_classes(12).tolist()) == set(range(7))
    with pytest.raises(AssertionError):
        T.bn_state(5, torch.Generator().manual_seed(1), "signed")           # no class 5 / 6, no dead channel before c = 5
    with pytest.raises(AssertionError):
        T.saturating(torch.tensor([25.0]))


@pytest.mark.parametrize("which", ["signed", "zero_init_residual"])
def test_gate_pinned_anchor_on_bn_states(which):
    """test_gate_pinned_fp32_vs_fp64_anchor for the whole-network cases of tests/test_gate_pinned_gpu.py on BatchNorm states with
    negative / zero / saturated gamma and zero-variance channels ("signed"), and with every bn3.weight = 0 ("zero_init_residual"): the
    same numbers (osi_testlib.network_case: B = 4, 64 x 64, C = 10), torch-CPU fp32 against fp64 with the fp64 run's decisions pinned.
    Measured, relative L2 per tensor over the tensors whose fp64 gradient is not identically 0:
        signed              median 2.4e-5, max 3.6e-5 (layer4.2.bn2.weight); 0 of 2 940 928 ReLU decisions and 0 arg-max positions flip
        zero_init_residual  median 1.7e-6, max 3.6e-6 (layer3.5.bn3.bias);   1 ReLU decision flips; 112 identically zero gradients
    Both maxima are below a third of 5e-4 (the headroom GRAD_TOL has over its original anchor), so the GPU tests keep GRAD_TOL = 5e-4.
    Conditions of the GPU tests checked here for the chosen seeds: the flip counts stay within the GPU tests' caps; fp32 reproduces the
    identically zero gradients exactly; in the signed case the saturated classes saturate (|0.05 xhat| < 1 everywhere: every bn1 / bn2 /
    stem gate of classes 3 and 5 off, of classes 2 and 4 on) and max |logit| in eval mode stays O(1), so LOGIT_TOL is absolute."""
    import osi_testlib as T
    sd, x, y = T.network_case(which)
    fn = lambda lg, t, f: L.entropic_openset_loss(lg, t, 1.0)
    sd64 = lambda: {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    rec64, rec32 = {}, {}
    r64 = R.forward_backward(sd64(), x.double(), y, fn, record_gates=rec64)
    R.forward_backward({k: v.clone() for k, v in sd.items()}, x, y, fn, record_gates=rec32)
    r32p = R.forward_backward({k: v.clone() for k, v in sd.items()}, x, y, fn, gates=rec64)
    flips, pool_flips, total = R.gate_disagreements(rec32, rec64)
    assert flips <= 2e-5 * total + 20 and pool_flips <= 2e-5 * rec64["pool_idx"].numel() + 5
    zeros = [k for k in r64[3] if float(r64[3][k].abs().max()) == 0]
    assert all(float(r32p[3][k].abs().max()) == 0 for k in zeros)
    pinned = {k: float((r32p[3][k].double() - r64[3][k]).norm() / r64[3][k].norm()) for k in r64[3] if k not in zeros}
    print(f"{which}: pinned median {np.median(list(pinned.values())):.2e} max {max(pinned.values()):.2e} flips {flips}/{total} pool {pool_flips} "
          f"zero tensors {len(zeros)}")
    assert len(pinned) + len(zeros) == 162 and len(zeros) == (0 if which == "signed" else 112)
    assert float((r32p[0].double() - r64[0]).abs().max()) <= 1e-5
    assert np.median(list(pinned.values())) <= 1e-4 and max(pinned.values()) <= 5e-4 / 3
    if which == "signed":
        for rec in (rec64, rec32):
            for i, g in enumerate(rec["relu"]):
                if i % 3 != 0 or i == 0:
                    T.assert_signed_gates(g.permute(0, 2, 3, 1), g.shape[1], f"gate {i}")
        with torch.no_grad():
            lg, _ = R.forward(sd64(), x.double(), training=False)
        assert float(lg.abs().max()) <= 4.0

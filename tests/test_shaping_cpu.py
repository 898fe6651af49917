"""CPU side of activation shaping (openset_imagenet/shaping.py, include/osi.h ABI 27): the oracle the GPU tests compare against
(tests/shaping_oracle.py) agrees with hand-worked rows, with np.percentile and with torch.topk where there are no ties; the symbols are
exported and declared; every C ABI entry validates its arguments before any launch; ActivationShaping refuses bad arguments by name
without a GPU; the data-free methods fit and round-trip their state on the CPU; evaluate.py takes and refuses the options."""
import ctypes

import numpy as np
import pytest
import torch

import shaping_oracle as O

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------- oracle
def test_oracle_on_hand_worked_rows():
    row = np.array([[0, 3, 0, 1, 0, 2]], dtype=np.float32)              # zeros straddle the cut at keep = 4: column 0 stays, 2 and 4 go
    assert O.kept_set(row[0], 4).tolist() == [True, True, False, True, False, True]
    assert O.kept_set(row[0], 3).tolist() == [False, True, False, True, False, True]
    assert O.kept_set(row[0], 6).all() and O.kept_set(row[0], 1).tolist() == [False, True, False, False, False, False]
    out, mask = O.shape_rows(row, O.ASH_P, 4)
    assert out.tolist() == row.tolist() and mask[0].tolist() == [True, True, False, True, False, True]
    out, _ = O.shape_rows(row, O.ASH_B, 4)
    assert out.tolist() == [[1.5, 1.5, 0, 1.5, 0, 1.5]]                 # s1 / keep = 6 / 4 on the kept set, zeros included
    out, _ = O.shape_rows(row, O.ASH_S, 2)                              # s1 / s2 = 6 / 5
    e = np.float32(np.exp(1.2))
    assert out.tolist() == [[0, np.float32(3) * e, 0, 0, 0, np.float32(2) * e]]
    out, mask = O.shape_rows(row, O.SCALE, 2)
    assert out.tolist() == (row * e).tolist() and mask.all()
    out, _ = O.shape_rows(np.array([[0.5, NAN, 2, -1]], dtype=np.float32), O.REACT, 0, 1.0)
    assert out[0, [0, 2, 3]].tolist() == [0.5, 1.0, -1.0] and np.isnan(out[0, 1])
    equal = np.full((1, 4), 5, dtype=np.float32)                        # an all-equal row: the lowest columns stay
    assert O.kept_set(equal[0], 2).tolist() == [True, True, False, False]
    out, _ = O.shape_rows(equal, O.ASH_B, 2)
    assert out.tolist() == [[10, 10, 0, 0]]
    out, _ = O.shape_rows(equal, O.ASH_S, 2)
    assert out.tolist() == [[np.float32(5) * np.float32(np.exp(2.0))] * 2 + [0, 0]]
    zeros = np.zeros((1, 3), dtype=np.float32)                          # 0 / 0: the IEEE result, not a special case
    assert np.isnan(O.shape_rows(zeros, O.SCALE, 1)[0]).all()
    out, _ = O.shape_rows(zeros, O.ASH_S, 1)
    assert np.isnan(out[0, 0]) and out[0, 1:].tolist() == [0, 0]
    special = np.array([1, NAN, INF, -0.0, 0.0, -INF, NAN], dtype=np.float32)
    assert O.kept_set(special, 3).tolist() == [False, True, True, False, False, False, True]          # NaN before +Inf, by column
    assert O.kept_set(special, 5).tolist() == [True, True, True, True, False, False, True]            # -0 = +0: the lower column
    assert O.ascending(special).tolist() == [5, 3, 4, 0, 2, 1, 6]
    got = O.order_stats(special, [0, 1, 2, 4, 6])
    assert got[:4].tolist() == [-INF, 0, 0, INF] and not np.signbit(got[1]) and np.isnan(got[4])


def test_oracle_percentile_against_numpy():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 1000):
        v = rng.standard_normal(n).astype(np.float32)
        for p in (0.001, 10.0, 50.0, 90.0, 99.9):
            want = np.percentile(v.astype(np.float64), p)
            got, j, count = O.linear_percentile(v, p)
            assert count == n and 0 <= j < n and np.isclose(got, want, rtol=1e-12, atol=1e-300), (n, p)
    assert O.linear_percentile(np.array([1, 2, 3, 4], dtype=np.float32), 50.0)[0] == 2.5


@pytest.mark.parametrize("f,keep", ((1, 1), (7, 3), (300, 30), (2048, 205)))
def test_oracle_kept_set_against_topk_without_ties(f, keep):
    rng = np.random.default_rng(f)
    row = rng.permutation(f).astype(np.float32) - f // 2                # distinct values
    want = np.zeros(f, dtype=bool)
    want[torch.topk(torch.from_numpy(row), keep).indices.numpy()] = True
    assert np.array_equal(O.kept_set(row, keep), want)


def test_oracle_scores():
    lg = np.array([[0, 0], [-INF, -INF], [1, NAN], [80, 80], [INF, 0]], dtype=np.float32)
    e, m, p = (O.logit_scores(lg, mode) for mode in (O.ENERGY, O.MAXLOGIT, O.MSP))
    assert e[0] == np.log(2.0) and e[1] == -INF and np.isnan(e[2]) and e[3] == 80 + np.log(2.0) and e[4] == INF
    assert m[[0, 1, 3, 4]].tolist() == [0, -INF, 80, INF] and np.isnan(m[2])
    assert p[0] == 0.5 and np.isnan(p[1]) and np.isnan(p[2]) and p[3] == 0.5 and np.isnan(p[4])
    assert O.ulps(np.float32([1, -0.0, NAN, 1]), np.float32([1 + 2 ** -23, 0.0, NAN, NAN])).tolist() == [1, 0, 0, 1 << 40]


def test_keep_rule():
    from openset_imagenet.shaping import ActivationShaping, keep_of
    assert (keep_of(1, 40), keep_of(2, 20), keep_of(2, 25), keep_of(2, 50), keep_of(2048, 90), keep_of(2048, 65)) == (1, 2, 2, 1, 205, 717)
    assert keep_of(2048, 90) == O.keep_of(2048, 90) and keep_of(2048, 60) == 2048 - 1229
    for width, p in ((1, 60), (1, 99), (2, 75), (2, 99.9), (2048, 99.99)):        # round(width p / 100) = width: nothing would stay
        assert O.keep_of(width, p) == 0
        with pytest.raises(ValueError, match="at least 1 must stay"):
            keep_of(width, p)
    assert ActivationShaping("react").keep(2048) == 0 and ActivationShaping("ash_s", 90).keep(2048) == 205


# ------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("osi_resnet50_pooled", "osi_order_stats_workspace", "osi_order_stats_f32", "osi_shape_rows_workspace", "osi_shape_rows",
         "osi_logit_scores")


def test_symbols_are_exported_and_declared():
    from openset_imagenet import _native as N
    lib = N.lib()
    assert lib.osi_abi_version() >= 27
    for name in NAMES:
        assert hasattr(lib, name) and name in N.declared_symbols()
    assert (N.SHAPE_REACT, N.SHAPE_ASH_P, N.SHAPE_ASH_B, N.SHAPE_ASH_S, N.SHAPE_SCALE) == (O.REACT, O.ASH_P, O.ASH_B, O.ASH_S, O.SCALE)
    assert (N.SCORE_ENERGY, N.SCORE_MAXLOGIT, N.SCORE_MSP) == (O.ENERGY, O.MAXLOGIT, O.MSP) == (0, 1, 2)
    assert N.ORDER_STATS_MAX_R == O.MAX_R == 8 and N.SHAPE_MAX_F == O.MAX_F == 4096
    ops = N.ops()
    for name in ("resnet50_pooled", "order_stats", "shape_rows", "logit_scores"):
        assert hasattr(ops, name)


def test_abi_entries_validate_before_launch():
    """Each null required pointer, a size <= 0 or past its limit, a bad enum, a rank outside [0, n), a keep outside its range, aliased
    rows, a workspace one byte short, absent or misaligned: OSI_ERR_ARG, nothing launched (safe on a CPU-only host; the device pointers
    are never dereferenced on the host - `ranks` is a host array and is a real one here)."""
    from openset_imagenet import _native as N
    lib = N.lib()
    for args in ((0, 2), (-5, 2), (100, 0), (100, -1), (100, N.ORDER_STATS_MAX_R + 1)):
        assert lib.osi_order_stats_workspace(*args) == 0, args
    nb = lib.osi_order_stats_workspace(100, 2)
    assert nb > 0 and nb % 8 == 0 and lib.osi_order_stats_workspace(1 << 40, 2) == nb < lib.osi_order_stats_workspace(100, 8)
    for args in ((0, 8), (-1, 8), (4, 0), (4, -2), (4, N.SHAPE_MAX_F + 1)):
        assert lib.osi_shape_rows_workspace(*args) == 0, args
    sb = lib.osi_shape_rows_workspace(65, 2048)
    assert sb > 0 and sb % 8 == 0
    p = 1 << 20                                           # any non-null, aligned address: argument checks come first

    def refuses(fn, good, pointers, values):
        for hole in pointers:
            args = list(good); args[hole] = None
            assert fn(*args) == -1, (fn.__name__, hole)
        for pos, value in values:
            args = list(good); args[pos] = value
            assert fn(*args) == -1, (fn.__name__, pos, value)

    ranks = lambda *r: (ctypes.c_longlong * len(r))(*r)
    refuses(lib.osi_order_stats_f32, [p, 100, ranks(0, 99), 2, p, p, nb, None], (0, 2, 4, 5),
            ((1, 0), (1, -1), (3, 0), (3, -1), (3, N.ORDER_STATS_MAX_R + 1), (2, ranks(0, 100)), (2, ranks(-1, 5)), (2, ranks(7, 1 << 40)),
             (6, nb - 1), (6, 0), (5, p + 4), (0, p + 2)))
    assert lib.osi_order_stats_f32(p, 100, ranks(*range(8)), 8, p, p, nb, None) == -1          # the workspace of two ranks is short for eight
    good = [p, 65, 2048, N.SHAPE_ASH_S, 205, 0.0, p + (1 << 24), p + (1 << 26), sb, None]
    refuses(lib.osi_shape_rows, good, (0, 6, 7),
            ((1, 0), (1, -1), (2, 0), (2, -1), (2, N.SHAPE_MAX_F + 1), (3, -1), (3, 5), (4, 0), (4, -1), (4, 2049), (8, sb - 1), (8, 0),
             (7, p + (1 << 26) + 4), (6, p), (6, p + 4 * 2048), (6, p + 4 * (65 * 2048 - 1)), (0, p + 2), (6, p + (1 << 24) + 2)))
    react = [p, 65, 2048, N.SHAPE_REACT, 0, 1.5, p + (1 << 24), p + (1 << 26), sb, None]
    for pos, value in ((4, 1), (4, -1), (4, 2048), (0, None), (6, None), (7, None), (6, p), (8, 0)):   # react prunes nothing: keep must be 0
        args = list(react); args[pos] = value
        assert lib.osi_shape_rows(*args) == -1, (pos, value)
    refuses(lib.osi_logit_scores, [p, 5, 7, N.SCORE_ENERGY, p, None], (0, 4),
            ((1, 0), (1, -1), (2, 0), (2, -1), (3, -1), (3, 3), (0, p + 2), (4, p + 1)))
    floats = ctypes.c_size_t(0)
    assert lib.osi_resnet50_pooled(None, p, p, ctypes.byref(floats), None) == -1


def test_pooled_accessor_reports_its_size_and_its_state_without_a_gpu():
    """The executor is a host object: before any forward the size query answers and a copy is refused (OSI_ERR_STATE), nothing launched."""
    from openset_imagenet import _native as N
    lib = N.lib()
    net = ctypes.c_void_p()
    assert lib.osi_resnet50_create(ctypes.byref(net), 3, 64, 64, 12, 7, 0) == 0
    try:
        floats = ctypes.c_size_t(0)
        assert lib.osi_resnet50_pooled(net, None, None, ctypes.byref(floats), None) == 0 and floats.value == 3 * 2048
        assert lib.osi_resnet50_pooled(net, None, None, None, None) == -1
        assert lib.osi_resnet50_pooled(net, None, 4096, ctypes.byref(floats), None) == -1        # a copy needs the workspace
        assert lib.osi_resnet50_pooled(net, 4096, 8192, ctypes.byref(floats), None) == -3        # ... and a forward
    finally:
        lib.osi_resnet50_destroy(net)


# ---------------------------------------------------------------------------------------------------------------- Python
def hand_head(p=6, f=4, c=3, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(f, p, generator=g), torch.randn(f, generator=g), torch.randn(c, f, generator=g),
            torch.randn(c, generator=g) if bias else None)


def test_names_import_and_refuse_without_gpu():
    import openset_imagenet
    from openset_imagenet.shaping import ActivationShaping, head_of
    from openset_imagenet.script.evaluate import shaping_arrays
    assert openset_imagenet.ActivationShaping is ActivationShaping and "ActivationShaping" in openset_imagenet.__all__
    head = hand_head()
    x = np.abs(np.random.default_rng(0).standard_normal((9, 6))).astype(np.float32)
    gt = np.array([0, 1, 2, -1, 0, 1, 2, -2, 0])
    fitted = ActivationShaping("ash_s", 50).fit(None, head=head)
    if torch.cuda.is_available():                        # with a GPU present they simply answer
        assert ActivationShaping("react").fit(x, gt, head=head).count == 7 and fitted.predict(x).shape == (9, 3)
    else:
        arrays = dict(gt=gt, pooled=x, logits=np.zeros((9, 3), np.float32), features=np.zeros((9, 4), np.float32))
        for call in (lambda: ActivationShaping("react").fit(x, gt, head=head), lambda: fitted.shape(x), lambda: fitted.logits(x),
                     lambda: fitted.predict(x), lambda: fitted.unknown_score(x), lambda: fitted.energy(x), lambda: fitted.max_logit(x),
                     lambda: fitted.msp(x), lambda: shaping_arrays(arrays, arrays, head, "scale", 50)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call()
    with pytest.raises(TypeError, match="a ResNet50 is expected"):
        head_of(torch.nn.Linear(3, 2))


def test_host_side_checks_name_the_argument():
    from openset_imagenet.shaping import ActivationShaping, DEFAULT_PERCENTILE, METHODS
    assert METHODS == O.MODES and set(DEFAULT_PERCENTILE) == set(METHODS)
    for bad in ("dice", "", "ReAct"):
        with pytest.raises(ValueError, match="method must be"):
            ActivationShaping(bad)
    for bad in (None, 0, 1.5, ["react"]):
        with pytest.raises(TypeError, match="method must be"):
            ActivationShaping(bad)
    for bad in (0, 100, -1, 100.5, NAN, INF):
        with pytest.raises(ValueError, match="0 < percentile < 100"):
            ActivationShaping("react", bad)
    for bad in ("90", True, [90], 1j):
        with pytest.raises(TypeError, match="percentile must be"):
            ActivationShaping("ash_p", bad)
    s = ActivationShaping("ash_b", np.float32(62.5))
    assert s.percentile == 62.5 and s.method == "ash_b" and not s.is_fitted and s.clip is None and s.count is None
    assert ActivationShaping("scale").percentile == DEFAULT_PERCENTILE["scale"]
    x = np.ones((5, 6), dtype=np.float32)
    for call, what in ((lambda: s.shape(x), "shape"), (lambda: s.logits(x), "logits"), (lambda: s.predict(x), "predict"),
                       (lambda: s.unknown_score(x), "unknown_score"), (lambda: s.energy(x), "energy"), (lambda: s.max_logit(x), "max_logit"),
                       (lambda: s.msp(x), "msp"), (lambda: s.state_dict(), "state_dict")):
        with pytest.raises(ValueError, match=f"{what} before fit"):
            call()
    head = hand_head()
    with pytest.raises(TypeError, match="head"):
        s.fit(None)
    for bad in (None, head[:3], list(head) + [None], "head", (None,) + head[1:], head[:2] + (None, None)):
        with pytest.raises(TypeError, match="head must be|head: fc_weight"):
            s.fit(None, head=bad)
    with pytest.raises(ValueError, match=r"fc_weight must be a matrix"):
        s.fit(None, head=(head[0][0],) + head[1:])
    with pytest.raises(ValueError, match=r"at most 4096"):
        s.fit(None, head=(torch.zeros(4, 4097),) + head[1:])
    with pytest.raises(ValueError, match=r"fc_bias must be \[4\]"):
        s.fit(None, head=(head[0], torch.zeros(5)) + head[2:])
    with pytest.raises(ValueError, match=r"logit_weight must be \[C, 4\]"):
        s.fit(None, head=head[:2] + (torch.zeros(3, 5), None))
    with pytest.raises(ValueError, match=r"logit_bias must be \[3\]"):
        s.fit(None, head=head[:3] + (torch.zeros(4),))
    with pytest.raises(ValueError, match="chunk must"):
        s.fit(None, head=head, chunk=0)
    with pytest.raises(ValueError, match=r"pooled must be \[N, 6\]"):
        s.fit(np.ones((5, 7), np.float32), head=head)
    with pytest.raises(ValueError, match=r"pooled must be \[N, 6\]"):
        s.fit(np.ones(6, np.float32), head=head)
    with pytest.raises(ValueError, match="at least 1 must stay"):
        ActivationShaping("ash_p", 99).fit(None, head=head)               # 6 - round(5.94) = 0
    react = ActivationShaping("react")
    for bad in (None, np.ones((0, 6), np.float32)):
        with pytest.raises(ValueError, match="react needs the pooled activations"):
            react.fit(bad, head=head)
    with pytest.raises(ValueError, match="disagree on the number of samples"):
        react.fit(x, np.zeros(4), head=head)
    with pytest.raises(ValueError, match="gt must be a vector"):
        react.fit(x, np.zeros((5, 1)), head=head)
    assert not react.is_fitted and not s.is_fitted
    s.fit(None, head=head)
    with pytest.raises(ValueError, match=r"pooled must be \[M, 6\]"):
        s.shape(np.ones((5, 7), np.float32))
    with pytest.raises(ValueError, match=r"pooled must be \[M, 6\]"):
        s.energy(np.ones(6, np.float32))
    with pytest.raises(ValueError, match="chunk must"):
        s.predict(x, chunk=-2)
    with pytest.raises(ValueError, match="chunk must"):
        s.unknown_score(x, chunk=1.5)


@pytest.mark.parametrize("method", ("ash_p", "ash_b", "ash_s", "scale"))
def test_data_free_fit_and_state_dict_round_trip_on_the_cpu(method):
    from openset_imagenet.shaping import ActivationShaping
    head = hand_head(bias=method != "ash_b")
    s = ActivationShaping(method, 50).fit(None, head=head)
    assert s.is_fitted and s.clip is None and s.count is None and s.fc_weight.device.type == "cpu" and s.keep(6) == 3
    assert s.fc_weight.data_ptr() != head[0].data_ptr() and (s.logit_bias is None) == (head[3] is None)
    sd = s.state_dict()
    assert set(sd) == {"fc_weight", "fc_bias", "logit_weight", "logit_bias", "method", "percentile", "clip", "count"}
    assert (sd["method"], sd["percentile"], sd["clip"], sd["count"]) == (method, 50.0, None, None)
    back = ActivationShaping("react", 10).load_state_dict(sd)
    assert (back.method, back.percentile, back.clip, back.count) == (method, 50.0, None, None)
    for k, want in zip(("fc_weight", "fc_bias", "logit_weight", "logit_bias"), head):
        got = getattr(back, k)
        assert (got is None and want is None) or (torch.equal(got, want) and got.dtype == torch.float32)
    for drop in ("fc_weight", "logit_bias", "method", "clip"):
        with pytest.raises(ValueError, match="lacks"):
            ActivationShaping(method).load_state_dict({k: v for k, v in sd.items() if k != drop})
    with pytest.raises(ValueError, match="holds no tensor"):
        ActivationShaping(method).load_state_dict(dict(sd, fc_bias=None))
    with pytest.raises(ValueError, match=r"fc_bias must be \[4\]"):
        ActivationShaping(method).load_state_dict(dict(sd, fc_bias=torch.zeros(3)))
    with pytest.raises(ValueError, match="method must be"):
        ActivationShaping(method).load_state_dict(dict(sd, method="dice"))
    with pytest.raises(ValueError, match="0 < percentile < 100"):
        ActivationShaping(method).load_state_dict(dict(sd, percentile=100))
    with pytest.raises(ValueError, match="at least 1 must stay"):
        ActivationShaping(method).load_state_dict(dict(sd, percentile=99))
    for clip in (None, NAN, INF):
        with pytest.raises(ValueError, match="react needs a finite clip"):
            ActivationShaping(method).load_state_dict(dict(sd, method="react", clip=clip))
    react = ActivationShaping(method).load_state_dict(dict(sd, method="react", clip=0.75, count=11))
    assert (react.method, react.clip, react.count) == ("react", 0.75, 11) and react.state_dict()["clip"] == 0.75


def test_evaluate_takes_and_refuses_the_options():
    from openset_imagenet.script.evaluate import DETECTORS, get_args
    a = get_args(["entropic", "2"])
    assert a.shaping is None and a.shaping_percentile is None
    a = get_args(["softmax", "1", "--shaping", "ash_s", "--shaping-percentile", "87.5", "--vim"])
    assert a.shaping == "ash_s" and a.shaping_percentile == 87.5 and a.vim is True
    assert [row["name"] for row in DETECTORS][-1] == "shaping" and DETECTORS[-1]["on"](a) and not DETECTORS[-1]["on"](get_args(["softmax", "1"]))
    assert DETECTORS[-1]["options"](a) == dict(method="ash_s", percentile=87.5)
    for bad in (["garbage", "1", "--shaping", "react"], ["softmax", "1", "--shaping", "dice"], ["softmax", "1", "--shaping"],
                ["softmax", "1", "--shaping", "react", "--shaping-percentile", "100"], ["softmax", "1", "--shaping-percentile", "0"],
                ["softmax", "1", "--shaping-percentile", "-3"], ["softmax", "1", "--shaping", "scale", "--shaping-percentile", "abc"],
                ["softmax", "1", "--shaping-percentile", "nan"]):
        with pytest.raises(SystemExit):
            get_args(bad)

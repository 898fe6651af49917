"""Configuration container with the semantics of the reference's util.NameSpace / util.load_yaml
(openset_imagenet/util.py:16-34): attribute access over a nested YAML mapping, `dump()` back to YAML text.
`calculate_oscr` mirrors util.py:90-122 on the GPU (osi_oscr_*). `get_histogram` mirrors util.py:202-228 (the score and
feature-norm histograms of known against negative / unknown samples): values, ranges and counts come from the GPU
(osi_eval_values_*, osi_hist_*), the bin edges from numpy on the host, and the four returned arrays carry the reference's values
and dtypes. `nearest_fpr` / `ccr_at_fpr` are the "CCR at FPR" rule of the reference's table (script/plot_all.py:344-385).
`oscr_by_rejection` (this build's addition) is the OSCR curve with a detector's `unknown` vector as the rejector (osi_det_*), `oscr_area`
the trapezoid area of either curve.
Drawing (matplotlib, PDF pages, TensorBoard event files) stays out of scope.
"""
import operator

import yaml


class NameSpace:
    def __init__(self, config):
        self.update(config)

    def update(self, config):
        for key, value in config.items():
            setattr(self, key, NameSpace(value) if isinstance(value, dict) else value)

    def dict(self):
        return {k: (v.dict() if isinstance(v, NameSpace) else v) for k, v in vars(self).items()}

    def dump(self, indent=4):
        return yaml.dump(self.dict(), indent=indent)

    def __repr__(self):
        return "NameSpace(" + repr(self.dict()) + ")"


def load_yaml(yaml_file):
    """Load a YAML configuration file into a NameSpace."""
    with open(yaml_file, "r") as handle:
        return NameSpace(yaml.safe_load(handle))


def calculate_oscr(gt, scores, unk_label=-1):
    """OSCR curve with the signature and return values of the reference (util.py:90-122): two float64 arrays (ccr, fpr), one
    point per distinct target-class score of the known samples except the largest.

    The counting runs on the MI355X (osi_oscr_f32 / osi_oscr_f64, exact integer counts, so the quotients are bit-identical to
    the reference's); `gt` / `scores` may be numpy arrays or torch tensors, on the host or already on the device (what
    validate()/get_arrays() hold). Score dtype float32 or float64 is kept — thresholds compare in the dtype they were stored in."""
    import numpy as np
    import torch
    from . import _native as N
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if dev is None:
        raise RuntimeError("openset_imagenet (MI355X build) has no CPU path: calculate_oscr needs the GPU")
    s = torch.as_tensor(scores)
    if s.dtype not in (torch.float32, torch.float64):
        s = s.double()
    if s.dim() != 2:
        raise ValueError("scores must be [N_samples, N_classes]")
    s = s.to(dev).contiguous()
    y = torch.as_tensor(np.asarray(gt).astype(int) if not isinstance(gt, torch.Tensor) else gt).to(torch.int64).to(dev).contiguous()
    n, c = s.shape
    if y.numel() != n:
        raise ValueError("gt and scores disagree on the number of samples")
    if n == 0:
        return np.zeros(0), np.zeros(0)
    lib = N.lib()
    nb = lib.osi_oscr_workspace(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    taus = torch.empty(n, dtype=s.dtype, device=dev)
    ccr_c = torch.zeros(n, dtype=torch.int64, device=dev)
    fpr_c = torch.zeros(n, dtype=torch.int64, device=dev)
    totals = torch.zeros(3, dtype=torch.int64, device=dev)
    fn = lib.osi_oscr_f32 if s.dtype == torch.float32 else lib.osi_oscr_f64
    N.check(fn(N.ptr(s), N.ptr(y), n, c, int(unk_label), N.ptr(ws), nb, N.ptr(taus), N.ptr(ccr_c), N.ptr(fpr_c), N.ptr(totals),
               N.stream_of(s)), "osi_oscr")
    n_unique, total_kn, total_unk = (int(v) for v in totals.cpu())
    pts = max(0, n_unique - 1)
    with np.errstate(divide="ignore", invalid="ignore"):   # 0/0 -> nan like the reference when a class of samples is absent
        ccr = ccr_c[:pts].cpu().numpy() / np.int64(total_kn)
        fpr = fpr_c[:pts].cpu().numpy() / np.int64(total_unk)
    return np.asarray(ccr, dtype=np.float64), np.asarray(fpr, dtype=np.float64)


def oscr_by_rejection(gt, scores, unknown, unk_label=-1):
    """OSCR curve with a separate rejection score: (ccr, fpr) as calculate_oscr returns them (two float64 arrays, same order), where a
    sample is rejected by `unknown` [N] (higher = more unknown, the vector the post-hoc detectors write) instead of by its class score,
    and `scores` [N, C] only decides the closed-set prediction: a known row is correct when the first maximum of its scores is its
    label (a row holding a NaN score is not). One point per distinct `unknown` value of the known rows except the smallest, from the
    largest down: ccr = #{correct, unknown < t} / #known, fpr = #{gt == unk_label, unknown < t} / #{gt == unk_label}. With
    unknown = -scores.max(1) and every known row correct this is calculate_oscr(gt, scores) bit for bit.

    Counted on the MI355X (osi_det_ranks_* / osi_det_curve_*, csrc/detection.hip); inputs as calculate_oscr takes them.
    ValueError("Input contains NaN.") when `unknown` holds a NaN."""
    import numpy as np
    import torch
    from . import _native as N
    from . import metrics
    dev = _need_gpu("oscr_by_rejection")
    s = _matrix_on_device(scores, dev, "scores")
    y, u, _ = metrics._detection_inputs(gt, unknown, None, "oscr_by_rejection")
    n = u.numel()
    if s.shape[0] != n:
        raise ValueError("scores and unknown disagree on the number of samples")
    if n == 0:
        return np.zeros(0), np.zeros(0)
    if s.shape[1] == 0:
        correct = torch.zeros(n, dtype=torch.uint8, device=dev)
    else:
        cols = torch.arange(s.shape[1], device=dev).expand_as(s)
        first_max = torch.where(s == s.max(1, keepdim=True).values, cols, s.shape[1]).min(1).values     # C on a row holding a NaN
        correct = (first_max == y).to(torch.uint8)
    ranks, counts, ws = metrics._det_ranks_device(y, u, correct, unk_label)
    taus = torch.empty(n, dtype=u.dtype, device=dev)
    out = torch.empty(2 * n + 3 + 4, dtype=torch.int64, device=dev)          # ccr_count[N], fpr_count[N], totals[3], counts4
    out[2 * n + 3:] = counts
    fn = N.lib().osi_det_curve_f32 if u.dtype == torch.float32 else N.lib().osi_det_curve_f64
    N.check(fn(N.ptr(u), N.ptr(y), N.ptr(ranks), n, int(unk_label), N.ptr(ws), ws.numel(), N.ptr(taus), N.ptr(out), N.ptr(out[n:]),
               N.ptr(out[2 * n:]), N.stream_of(u)), "osi_det_curve")
    host = out.cpu().numpy()
    n_unique, total_kn, total_unk = (int(v) for v in host[2 * n:2 * n + 3])
    if host[2 * n + 6]:
        raise ValueError("Input contains NaN.")
    pts = max(0, n_unique - 1)
    with np.errstate(divide="ignore", invalid="ignore"):   # 0/0 -> nan as in calculate_oscr when a class of samples is absent
        ccr = host[:pts] / np.int64(total_kn)
        fpr = host[n:n + pts] / np.int64(total_unk)
    return np.asarray(ccr, dtype=np.float64), np.asarray(fpr, dtype=np.float64)


def oscr_area(ccr, fpr):
    """Area under an OSCR curve as calculate_oscr / oscr_by_rejection return it (fpr falls along the curve): the trapezoid sum of ccr
    over fpr between the curve's own end points, no extrapolation to fpr 0 or 1, on the host in fp64. 0.0 for fewer than two points,
    nan when a point is not finite (a split without known or without unknown rows)."""
    import numpy as np
    ccr, fpr = np.asarray(ccr, dtype=np.float64), np.asarray(fpr, dtype=np.float64)
    if ccr.shape != fpr.shape or ccr.ndim != 1:
        raise ValueError("ccr and fpr must be vectors of one length")
    if not (np.isfinite(ccr).all() and np.isfinite(fpr).all()):
        return float("nan")
    if len(ccr) < 2:
        return 0.0
    return float(np.sum((fpr[:-1] - fpr[1:]) * (ccr[:-1] + ccr[1:]) * 0.5))


def _need_gpu(what):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"openset_imagenet (MI355X build) has no CPU path: {what} needs the GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _matrix_on_device(x, dev, name):
    """[N, K] matrix on the device as calculate_oscr takes it: numpy or torch, host or device; fp32 / fp64 kept, anything else fp64."""
    import torch
    t = torch.as_tensor(x).detach()
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if t.dim() != 2:
        raise ValueError(f"{name} must be a matrix [N_samples, N_columns]")
    return t.to(dev).contiguous()


def _labels_on_device(gt, dev):
    import numpy as np
    import torch
    y = gt.detach() if isinstance(gt, torch.Tensor) else torch.as_tensor(np.asarray(gt).astype(int))
    return y.to(torch.int64).to(dev).contiguous()


def _eval_values(scores, features, gt, metric, unk_label, drop_last):
    """osi_eval_values_* on device tensors (`scores` or `features` may be None where the metric does not read it): the device
    tensors kn_val, unk_val, side and the host lists range4 (floats) and counts6 (ints). One copy to the host."""
    import torch
    from . import _native as N
    src = scores if metric == N.EVAL_SCORE else features
    n, dev, dt = src.shape[0], src.device, src.dtype
    lib = N.lib()
    nb = lib.osi_eval_values_workspace(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    kn_val, unk_val = torch.empty(n, dtype=dt, device=dev), torch.empty(n, dtype=dt, device=dev)
    side = torch.empty(n, dtype=torch.uint8, device=dev)
    out = torch.empty(10, dtype=torch.int64, device=dev)               # range4 as fp64 bits, then counts6
    fn = lib.osi_eval_values_f32 if dt == torch.float32 else lib.osi_eval_values_f64
    N.check(fn(N.ptr(scores), N.ptr(features), N.ptr(gt), n, 0 if scores is None else scores.shape[1],
               0 if features is None else features.shape[1], metric, int(unk_label), int(bool(drop_last)), N.ptr(kn_val),
               N.ptr(unk_val), N.ptr(side), N.ptr(out), N.ptr(out[4:]), N.ptr(ws), nb, N.stream_of(src)), "osi_eval_values")
    host = out.cpu()
    return kn_val, unk_val, side, host[:4].view(torch.float64).tolist(), host[4:].tolist()


def _hist_counts(val, side, side_bit, edges):
    """osi_hist_* on device tensors: the int64 counts (numpy) of the rows with side & side_bit over `edges` (numpy, any real dtype;
    uploaded as fp64)."""
    import numpy as np
    import torch
    from . import _native as N
    nb = len(edges) - 1
    if nb < 1 or val.numel() == 0:
        return np.zeros(max(nb, 0), dtype=np.int64)
    e = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).to(val.device)
    counts = torch.empty(nb, dtype=torch.int64, device=val.device)
    lib = N.lib()
    fn = lib.osi_hist_f32 if val.dtype == torch.float32 else lib.osi_hist_f64
    N.check(fn(N.ptr(val), N.ptr(side), side_bit, val.numel(), N.ptr(e), nb, N.ptr(counts), N.stream_of(val)), "osi_hist")
    return counts.cpu().numpy()


def get_histogram(array, unk_label=-1, metric='score', bins=100, drop_bg=False, log_space=False, geomspace_limits=(1, 1e2)):
    """Histograms of the scores or of the feature norms of known (gt >= 0) and of `unk_label` samples, with the signature and the
    return values of the reference (util.py:202-228): (kn_hist, kn_edges, unk_hist, unk_edges), int64 counts, edges in the data's
    dtype for an integer `bins` and float64 (what was passed) for `log_space` or a sequence of edges.

    `array` maps 'scores', 'gt' and, for metric='norm' only, 'features' to numpy arrays or torch tensors, on the host or on the
    device; `gt` may be float32 (what get_arrays returns). Known samples contribute scores[i, gt[i]], unknown ones the row maximum
    (drop_bg: without the last column). Values, their range and the counts come from the MI355X (osi_eval_values_*, osi_hist_*);
    the edges are numpy's, made on the host from the device's {min, max}: np.histogram_bin_edges of those two numbers is what
    np.histogram computes from the full data, widening of min == max and the [0, 1] range of an empty side included.

    Raises as numpy does: ValueError for a NaN or an infinity on a side when `bins` is an integer ("autodetected range ... is not
    finite") and for edges that decrease, IndexError for a known label beyond the class columns. Of its own: ValueError for more than
    4096 bins and for an unknown `metric` (the reference: UnboundLocalError); RuntimeError without a GPU. Norms are summed in fp64
    and rounded once, where the reference sums in the features' dtype (divergences)."""
    import numpy as np
    import torch
    from . import _native as N
    if metric not in ("score", "norm"):
        raise ValueError(f"metric must be 'score' or 'norm', not {metric!r}")
    if log_space:
        lower, upper = geomspace_limits
        bins = np.geomspace(lower, upper, num=bins)
    if isinstance(bins, str):
        raise ValueError("bin estimators by name are not supported: pass a bin count or the edges")
    try:
        n_bins, edges = operator.index(bins), None
        if n_bins < 1:
            raise ValueError("`bins` must be positive, when an integer")
    except TypeError:
        n_bins, edges = None, np.asarray(bins)
        if edges.ndim != 1:
            raise ValueError("`bins` must be 1d, when an array")
        if np.any(edges[:-1] > edges[1:]):
            raise ValueError("`bins` must increase monotonically, when an array")
    if (n_bins if edges is None else len(edges) - 1) > N.HIST_MAX_BINS:
        raise ValueError(f"more than {N.HIST_MAX_BINS} bins are not supported")
    dev = _need_gpu("get_histogram")
    y = _labels_on_device(array["gt"], dev)
    if metric == "score":
        s, f, code = _matrix_on_device(array["scores"], dev, "scores"), None, N.EVAL_SCORE
        classes = s.shape[1] - int(bool(drop_bg))
        if classes < 1:
            raise ValueError("scores hold no class column")
        src = s
    else:
        s, f, code = None, _matrix_on_device(array["features"], dev, "features"), N.EVAL_NORM
        if f.shape[1] < 1:
            raise ValueError("features hold no column")
        src = f
    if y.numel() != src.shape[0]:
        raise ValueError("gt and the data disagree on the number of samples")
    np_type = np.float32 if src.dtype == torch.float32 else np.float64
    if src.shape[0] == 0:
        kn_val = unk_val = torch.empty(0, dtype=src.dtype, device=dev)
        side, rng, cnt = torch.empty(0, dtype=torch.uint8, device=dev), [0.0] * 4, [0] * 6
    else:
        kn_val, unk_val, side, rng, cnt = _eval_values(s, f, y, code, unk_label, drop_bg)
    if cnt[4]:
        raise IndexError(f"{cnt[4]} known label(s) out of bounds for axis 1 with size {classes}")

    def side_edges(count, nans, lo, hi):
        if edges is not None:
            return edges
        if count == 0:
            return np.histogram_bin_edges(np.empty(0, dtype=np_type), n_bins)
        if nans:
            lo = hi = float("nan")
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"autodetected range of [{lo}, {hi}] is not finite")
        return np.histogram_bin_edges(np.array([lo, hi], dtype=np_type), n_bins)

    kn_edges = side_edges(cnt[0], cnt[2], rng[0], rng[1])
    kn_hist = _hist_counts(kn_val, side, 1, kn_edges)
    unk_edges = side_edges(cnt[1], cnt[3], rng[2], rng[3])
    unk_hist = _hist_counts(unk_val, side, 2, unk_edges)
    return kn_hist, kn_edges, unk_hist, unk_edges


def nearest_fpr(ccr, fpr, fpr_values=(1e-3, 1e-2, 0.1, 1.0), max_error=10.0):
    """The "CCR at FPR" rule of the reference's table (script/plot_all.py:346-384), host code: for each query q the curve point whose
    fpr is nearest to q (the first of several), and None ("---" in the table) when that fpr is off by `max_error` percent of q or more
    after rounding the percentage to one decimal. An empty curve gives None for every q (the reference would raise). Returns a list
    with one float or None per query."""
    import numpy as np
    ccr, fpr = np.asarray(ccr), np.asarray(fpr)
    out = []
    for q in fpr_values:
        if fpr.size == 0:
            out.append(None)
            continue
        idx = np.abs(fpr - q).argmin()
        error = round(100 * abs(fpr[idx] - q) / q, 1)
        out.append(None if error >= max_error else float(ccr[idx]))
    return out


def ccr_at_fpr(gt, scores, fpr_values=(1e-3, 1e-2, 0.1, 1.0), unk_label=-2, max_error=10.0):
    """calculate_oscr(gt, scores, unk_label) followed by nearest_fpr: the CCR columns of the reference's table row."""
    ccr, fpr = calculate_oscr(gt, scores, unk_label=unk_label)
    return nearest_fpr(ccr, fpr, fpr_values=fpr_values, max_error=max_error)

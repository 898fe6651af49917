"""The Extreme Value Machine (Rudd, Jain, Scheirer, Boult, "The Extreme Value Machine", TPAMI 2018) on the MI355X: the other post-hoc
open-set method beside OpenMax, on the features of a trained closed-set network.

    evm = EVM(tailsize=1000, cover_threshold=None, distance_multiplier=0.5, distance="cosine", use_negatives=True)
    evm.fit(features, gt)            # the arrays of train.get_arrays on the TRAINING split; classes = 0 .. max known label
    probs = evm.predict(features)    # [M, C] fp32 on the device

`fit` gives every training row of a known class a Weibull distribution over the (scaled) distances to its `tailsize` nearest
negatives - every row with another label, the negative (-1) samples included unless `use_negatives=False` - and, with a
`cover_threshold`, keeps per class only the rows a greedy set cover needs to explain the others (the extreme vectors); without one
every fitted row is an extreme vector. `predict` scores a class by the largest inclusion probability over its extreme vectors. The
method is not part of the reference snapshot: include/osi.h (ABI 22) is its definition, tests/evm_oracle.py its fp64 restatement.
`probs` feeds util.calculate_oscr, util.ccr_at_fpr and util.get_histogram as it is.

All arithmetic runs in the kernels of csrc/evm.hip (torch.ops.osi.evm_*): all-pairs distances on the fp32 matrix cores, one workgroup
per row for the fit. There is no CPU path. Inputs may be numpy arrays or torch tensors, on the host or on the device. `fit` takes the
labels to the host once, before its loop over the classes (they size the launches); inside the loop nothing is read back, and ONE
readback of the per-class extreme-vector counts at the end sizes the model: `ev_features [V, F]`, `ev_shape`, `ev_scale`, `ev_shift`
(one entry per extreme vector, sorted by class), `ev_start [C + 1]` and `flags` ({candidate distances left out as not finite,
unfitted rows}), device tensors the caller may read. Out of scope: per-class tail sizes, incremental updates, multi-GPU fitting.
"""
import numpy as np
import torch

from . import _native as N
from ._detector import _DESC_LIMIT, Detector, _check_chunk, _chunk_rows, _fit_shapes, _host_labels, _launch_rows, _matrix
from .util import _labels_on_device, _need_gpu

_METRICS = {"euclidean": N.EVM_EUCLIDEAN, "cosine": N.EVM_COSINE}


class EVM(Detector):
    _STATE = ("ev_features", "ev_shape", "ev_scale", "ev_shift", "ev_start", "flags")
    _SETTINGS = ("tailsize", "cover_threshold", "distance_multiplier", "distance", "use_negatives")
    _DTYPES = dict(ev_features=torch.float32, ev_shape=torch.float64, ev_scale=torch.float64, ev_shift=torch.float64,
                   ev_start=torch.int64, flags=torch.int64)

    def __init__(self, tailsize=1000, cover_threshold=None, distance_multiplier=0.5, distance="cosine", use_negatives=True):
        if isinstance(tailsize, bool) or not isinstance(tailsize, int):
            raise TypeError(f"tailsize must be an int, got {type(tailsize).__name__}")
        if not 2 <= tailsize <= N.EVM_MAX_TAIL:
            raise ValueError(f"tailsize must lie in [2, {N.EVM_MAX_TAIL}], got {tailsize}")
        if cover_threshold is not None:
            if isinstance(cover_threshold, bool) or not isinstance(cover_threshold, (int, float)):
                raise TypeError(f"cover_threshold must be a number or None, got {type(cover_threshold).__name__}")
            if not 0.0 <= cover_threshold <= 1.0:
                raise ValueError(f"cover_threshold must lie in [0, 1], got {cover_threshold}")
            cover_threshold = float(cover_threshold)
        if isinstance(distance_multiplier, bool) or not isinstance(distance_multiplier, (int, float)):
            raise TypeError(f"distance_multiplier must be a number, got {type(distance_multiplier).__name__}")
        with np.errstate(over="ignore", under="ignore"):
            m32 = np.float32(distance_multiplier)
        if not (distance_multiplier > 0 and np.isfinite(m32) and m32 > 0):
            raise ValueError(f"distance_multiplier must be positive and finite in fp32, got {distance_multiplier}")
        if distance not in _METRICS:
            raise ValueError(f"distance must be one of {sorted(_METRICS)}, got {distance!r}")
        self.tailsize, self.cover_threshold, self.distance_multiplier = tailsize, cover_threshold, float(distance_multiplier)
        self.distance, self.use_negatives = distance, bool(use_negatives)
        for name in self._STATE:
            setattr(self, name, None)
        self._ws = None

    # ---------------------------------------------------------------------------------------------------------------- fit
    def fit(self, features, gt):
        """One Weibull per row of a known class from features [N, F] and labels [N] of the training split; the extreme vectors of
        every class 0 .. max(gt). Rows with labels below 0 are negatives of every class (dropped when use_negatives is False).
        Returns self."""
        f_shape = _fit_shapes(features, gt)
        y_host = _host_labels(gt)
        c = int(y_host.max()) + 1
        keep = None
        if not self.use_negatives and (y_host < 0).any():
            keep = np.flatnonzero(y_host >= 0)
            y_host = y_host[keep]
        n, f_dim = len(y_host), f_shape[1]
        if n * f_dim * 4 >= _DESC_LIMIT:
            raise ValueError(f"features of {n} rows x {f_dim} columns reach the 2 GiB limit of the distance kernel (N * F * 4 >= 2^31)")
        rows = [np.flatnonzero(y_host == k) for k in range(c)]
        if self.cover_threshold is not None:
            for k, idx in enumerate(rows):
                if len(idx) > N.EVM_MAX_COVER_ROWS:
                    raise ValueError(f"class {k} has {len(idx)} rows, more than the {N.EVM_MAX_COVER_ROWS} the set cover takes: "
                                     f"fit without cover_threshold or subsample the class")
        dev = _need_gpu("EVM.fit")
        ops = N.ops()
        f = _matrix(features, dev, "features")
        if keep is not None:
            f = f[torch.from_numpy(keep).to(dev)].contiguous()
        y = _labels_on_device(y_host, dev)
        metric, mult = _METRICS[self.distance], self.distance_multiplier
        step = _chunk_rows(n)
        ws = self._workspace(N.lib().osi_evm_workspace(max(len(i) for i in rows), n, f_dim), dev)
        per_class, flags = [], torch.zeros(2, dtype=torch.int64, device=dev)
        for k, idx in enumerate(rows):                          # nothing is read back in here
            if len(idx) == 0:
                per_class.append(None)
                continue
            x = f[torch.from_numpy(idx).to(dev)].contiguous()
            parts = []
            for r0 in range(0, len(idx), step):
                dist = ops.evm_distances(x[r0:r0 + step], f, metric, ws)
                parts.append(ops.evm_fit_rows(dist, y, k, self.tailsize, mult, ws))
                flags = flags + parts[-1][5]
                del dist
            shape, scale, shift, fitted = (torch.cat([p[j] for p in parts]) for j in range(4))
            if self.cover_threshold is not None:
                dpp = ops.evm_distances(x, x, metric, ws)
                order, n_ev = ops.evm_set_cover(dpp, shape, scale, shift, fitted, mult, self.cover_threshold, ws)
                del dpp
            else:                                               # every fitted row, in row order
                order = torch.argsort(fitted == 0, stable=True)
                n_ev = (fitted != 0).sum().reshape(1)
            per_class.append((x, shape, scale, shift, order, n_ev))
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        counts = torch.cat([zero if p is None else p[5] for p in per_class]).cpu().tolist()       # the one readback
        ev = [[], [], [], []]
        for p, m in zip(per_class, counts):
            if m:
                sel = p[4][:m]
                for j in range(4):
                    ev[j].append(p[j][sel])
        if ev[0]:
            self.ev_features, self.ev_shape, self.ev_scale, self.ev_shift = (torch.cat(e).contiguous() for e in ev)
        else:
            self.ev_features = torch.empty(0, f_dim, dtype=torch.float32, device=dev)
            self.ev_shape, self.ev_scale, self.ev_shift = (torch.empty(0, dtype=torch.float64, device=dev) for _ in range(3))
        self.ev_start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), device=dev)
        self.flags = flags
        return self

    # ------------------------------------------------------------------------------------------------------------ predict
    def predict(self, features, chunk=None):
        """[M, C] fp32 on the device: per class the largest inclusion probability over its extreme vectors (0 for a class without
        any). `chunk`: query rows per launch (default: as many as the 2 GiB limit of a distance matrix allows)."""
        self._require_fit("predict")
        f_shape = tuple(torch.as_tensor(features).shape)
        v, f_dim = self.ev_features.shape
        c = self.ev_start.numel() - 1
        if len(f_shape) != 2 or f_shape[1] != f_dim:
            raise ValueError(f"features must be [M, {f_dim}] (the width fit saw), got shape {f_shape}")
        _check_chunk(chunk)
        dev = _need_gpu("EVM.predict")
        self._on(dev)
        m = f_shape[0]
        if m == 0 or v == 0:
            return torch.zeros(m, c, dtype=torch.float32, device=dev)
        step = min(_chunk_rows(v), _launch_rows(m, f_dim), chunk or m)
        ops = N.ops()
        q = _matrix(features, dev, "features")
        ws = self._workspace(N.lib().osi_evm_workspace(min(step, m), v, f_dim), dev)
        out = torch.empty(m, c, dtype=torch.float32, device=dev)
        for r0 in range(0, m, step):
            dist = ops.evm_distances(q[r0:r0 + step], self.ev_features, _METRICS[self.distance], ws)
            out[r0:r0 + step] = ops.evm_probs(dist, self.ev_shape, self.ev_scale, self.ev_shift, self.ev_start, self.distance_multiplier)
        return out

    # -------------------------------------------------------------------------------------------------------------- state
    def _restore(self, sd, tensors):
        cover = sd["cover_threshold"]
        EVM.__init__(self, int(sd["tailsize"]), None if cover is None else float(cover), float(sd["distance_multiplier"]), sd["distance"],
                     bool(sd["use_negatives"]))
        if tensors["ev_features"].dim() != 2:
            raise ValueError(f"state dict: ev_features must be [V, F], got shape {tuple(tensors['ev_features'].shape)}")
        v = tensors["ev_features"].shape[0]
        for k in ("ev_shape", "ev_scale", "ev_shift"):
            if tuple(tensors[k].shape) != (v,):
                raise ValueError(f"state dict: {k} must hold one entry per extreme vector ({v}), got shape {tuple(tensors[k].shape)}")
        start = tensors["ev_start"]
        if start.dim() != 1 or start.numel() < 2 or int(start[0]) != 0 or int(start[-1]) != v or bool((start[1:] < start[:-1]).any()):
            raise ValueError(f"state dict: ev_start must be [C + 1] offsets rising from 0 to {v}, got {start.tolist()}")
        if tuple(tensors["flags"].shape) != (2,):
            raise ValueError(f"state dict: flags must hold two entries, got shape {tuple(tensors['flags'].shape)}")

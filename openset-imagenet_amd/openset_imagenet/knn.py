"""Deep nearest neighbours (Sun, Ming, Zhu, Li, "Out-of-Distribution Detection with Deep Nearest Neighbors", ICML 2022) on the MI355X:
the non-parametric post-hoc open-set method beside OpenMax and the EVM, on the features of a trained closed-set network.

    knn = KNN(k=10, distance="cosine", bank_fraction=1.0, seed=0)
    knn.fit(features, gt)                    # the arrays of train.get_arrays on the TRAINING split; classes = 0 .. max known label
    scores = knn.predict(features)           # [M, C] fp32 on the device: per class the similarity of the k-th nearest bank row OF THAT CLASS
    unknown = knn.unknown_score(features)    # [M] fp32: the distance to the k-th nearest bank row overall (larger = more unknown)
    d, idx = knn.kneighbors(features)        # [M, k] each; idx are row numbers of the array fit() was given
    knn.calibrate(tpr=0.95)                  # leave-one-out unknown_score over the bank -> knn.threshold

`fit` keeps the rows of the known classes as the bank, sorted by class (a stable sort: row order is kept inside a class); rows with a
label below 0 are DROPPED - the negatives are not a scored segment. `bank_fraction < 1` keeps ceil(fraction * n_c) rows of every class,
drawn on the host from a torch.Generator seeded with `seed`: the same seed gives the same bank. The similarity of `predict` is
clamp(1 - d / 2, 0, 1) for the cosine distance and 1 / (1 + d) for the Euclidean one, so the scores lie in [0, 1] and feed
util.calculate_oscr, util.ccr_at_fpr and util.get_histogram as they are; a class without bank rows scores 0. With fewer than k rows in
a class (or in the bank) the farthest one stands in for the k-th. The method is not part of the reference snapshot: include/osi.h
(ABI 24) is its definition, tests/knn_oracle.py its numpy restatement.

Distances and selection run in the kernels of csrc/evm.hip and csrc/knn.hip (torch.ops.osi.evm_distances, knn_topk, knn_class_kth)
and nowhere else; there is no CPU path. Inputs may be numpy arrays or torch tensors, on the host or on the device. `fit` takes the
labels to the host once (the class counts size the bank); `predict`, `unknown_score` and `kneighbors` read nothing back. The fitted
state - `bank_features [N, F]`, `bank_start [C + 1]`, `bank_rows [N]` (the original row numbers), `bank_labels [N]` and, after
`calibrate`, `threshold` - are device tensors the caller may read. Out of scope: banks of 2 GiB and more (N * F * 4 >= 2^31 is refused;
lower `bank_fraction`), approximate search, multi-GPU banks."""
import math

import numpy as np
import torch

from . import _native as N
from ._detector import _DESC_LIMIT, Detector, _check_chunk, _chunk_rows, _fit_shapes, _host_labels, _launch_rows, _matrix
from .util import _labels_on_device, _need_gpu

_METRICS = {"euclidean": N.EVM_EUCLIDEAN, "cosine": N.EVM_COSINE}
_TRANSFORMS = {"euclidean": N.KNN_SIM_INVERSE, "cosine": N.KNN_SIM_COSINE}


def bank_selection(gt, bank_fraction=1.0, seed=0):
    """Host bookkeeping of fit: (rows, start) from the labels gt [N]. rows = the row numbers of the bank in bank order - sorted by
    class, ascending inside a class -, start [C + 1] = the class offsets into it, C = max(gt) + 1. Rows with gt < 0 are left out. With
    bank_fraction < 1 every class keeps ceil(bank_fraction * n_c) of its rows, drawn without replacement from one torch.Generator
    seeded with `seed` and walked over the classes in order."""
    y = np.asarray(gt).astype(np.int64)
    c = int(y.max()) + 1
    order = np.argsort(y, kind="stable")
    order = order[y[order] >= 0]
    counts = np.bincount(y[order], minlength=c)
    if bank_fraction < 1.0:
        gen = torch.Generator().manual_seed(int(seed))
        kept, first = [], 0
        for n_c in counts.tolist():
            take = math.ceil(bank_fraction * n_c)
            pick = np.sort(torch.randperm(n_c, generator=gen)[:take].numpy())
            kept.append(order[first:first + n_c][pick])
            first += n_c
        order = np.concatenate(kept) if kept else order[:0]
        counts = np.array([len(p) for p in kept], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return order.astype(np.int64), start


class KNN(Detector):
    _STATE = ("bank_features", "bank_start", "bank_rows", "bank_labels")
    _OPTIONAL = ("threshold",)
    _SETTINGS = ("k", "distance", "bank_fraction", "seed")
    _DTYPES = dict(bank_features=torch.float32, bank_start=torch.int64, bank_rows=torch.int64, bank_labels=torch.int64,
                   threshold=torch.float32)

    def __init__(self, k=10, distance="cosine", bank_fraction=1.0, seed=0):
        if isinstance(k, bool) or not isinstance(k, int):
            raise TypeError(f"k must be an int, got {type(k).__name__}")
        if not 1 <= k <= N.KNN_MAX_K:
            raise ValueError(f"k must lie in [1, {N.KNN_MAX_K}], got {k}")
        if distance not in _METRICS:
            raise ValueError(f"distance must be one of {sorted(_METRICS)}, got {distance!r}")
        if isinstance(bank_fraction, bool) or not isinstance(bank_fraction, (int, float)):
            raise TypeError(f"bank_fraction must be a number, got {type(bank_fraction).__name__}")
        if not 0.0 < bank_fraction <= 1.0:
            raise ValueError(f"bank_fraction must lie in (0, 1], got {bank_fraction}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError(f"seed must be an int, got {type(seed).__name__}")
        self.k, self.distance, self.bank_fraction, self.seed = k, distance, float(bank_fraction), seed
        for name in self._STATE + self._OPTIONAL:
            setattr(self, name, None)
        self._ws = None

    # ------------------------------------------------------------------------------------------------------------ helpers
    def _queries(self, features, chunk, what, exclude_self=False):
        """Checks of every scoring call, before any GPU work: (shape of the queries, device, rows per launch)."""
        self._require_fit(what)
        f_shape = tuple(torch.as_tensor(features).shape)
        n, f_dim = self.bank_features.shape
        if len(f_shape) != 2 or f_shape[1] != f_dim:
            raise ValueError(f"features must be [M, {f_dim}] (the width fit saw), got shape {f_shape}")
        _check_chunk(chunk)
        if exclude_self and f_shape[0] != n:
            raise ValueError(f"exclude_self=True takes the bank itself as queries ({n} rows, in bank order), got {f_shape[0]} rows")
        dev = _need_gpu(f"KNN.{what}")
        self._on(dev)
        m = f_shape[0]
        return m, dev, min(_chunk_rows(n), _launch_rows(m, f_dim), chunk or max(m, 1))

    def _chunks(self, q, m, step, dev):
        """(first row, distance chunk [rows, N]) over the query rows; the workspace is shared by all of them."""
        n, f_dim = self.bank_features.shape
        lib, rows = N.lib(), min(step, m)
        ws = self._workspace(max(lib.osi_evm_workspace(rows, n, f_dim), lib.osi_knn_workspace(rows, n, self.k)), dev)
        for r0 in range(0, m, step):
            yield r0, N.ops().evm_distances(q[r0:r0 + step], self.bank_features, _METRICS[self.distance], ws), ws

    # ---------------------------------------------------------------------------------------------------------------- fit
    def fit(self, features, gt):
        """The bank from features [N, F] and labels [N] of the training split: the rows of the classes 0 .. max(gt), sorted by class.
        Rows with labels below 0 (negatives) are dropped. Forgets an earlier calibration. Returns self."""
        f_shape = _fit_shapes(features, gt)
        y_host = _host_labels(gt)                           # the one readback
        rows, start = bank_selection(y_host, self.bank_fraction, self.seed)
        n, f_dim = len(rows), f_shape[1]
        if n * f_dim * 4 >= _DESC_LIMIT:
            raise ValueError(f"a bank of {n} rows x {f_dim} columns reaches the 2 GiB limit of the distance kernel (N * F * 4 >= 2^31): "
                             f"lower bank_fraction (now {self.bank_fraction})")
        dev = _need_gpu("KNN.fit")
        f = _matrix(features, dev, "features")
        self.bank_rows = torch.from_numpy(rows).to(dev)
        self.bank_features = f[self.bank_rows].contiguous()
        self.bank_start = torch.from_numpy(start).to(dev)
        self.bank_labels = _labels_on_device(y_host[rows], dev)
        self.threshold = None
        return self

    # ------------------------------------------------------------------------------------------------------------ scoring
    def predict(self, features, chunk=None):
        """[M, C] fp32 on the device: per class the similarity of the k-th nearest bank row of that class (0 for a class without bank
        rows). `chunk`: query rows per launch (default: as many as the 2 GiB limit of a distance matrix allows)."""
        m, dev, step = self._queries(features, chunk, "predict")
        c = self.bank_start.numel() - 1
        out = torch.empty(m, c, dtype=torch.float32, device=dev)
        if m == 0:
            return out
        q = _matrix(features, dev, "features")
        for r0, dist, ws in self._chunks(q, m, step, dev):
            out[r0:r0 + step] = N.ops().knn_class_kth(dist, self.bank_start, self.k, None, _TRANSFORMS[self.distance], ws)
        return out

    def _kth_overall(self, q, m, step, dev, leave_one_out):
        n = self.bank_features.shape[0]
        whole = torch.tensor([0, n], dtype=torch.int64, device=dev)
        out = torch.empty(m, dtype=torch.float32, device=dev)
        for r0, dist, ws in self._chunks(q, m, step, dev):
            skip = torch.arange(r0, r0 + dist.shape[0], dtype=torch.int64, device=dev) if leave_one_out else None
            out[r0:r0 + step] = N.ops().knn_class_kth(dist, whole, self.k, skip, N.KNN_RAW, ws).reshape(-1)
        return out

    def unknown_score(self, features, chunk=None):
        """[M] fp32 on the device: the distance to the k-th nearest bank row of any class (Sun et al.'s score; larger = more unknown)."""
        m, dev, step = self._queries(features, chunk, "unknown_score")
        if m == 0:
            return torch.empty(0, dtype=torch.float32, device=dev)
        return self._kth_overall(_matrix(features, dev, "features"), m, step, dev, False)

    def kneighbors(self, features, exclude_self=False, chunk=None):
        """(distances [M, k] fp32, rows [M, k] int64) on the device: the k nearest bank rows, nearest first, ties by bank position; rows
        are row numbers of the array fit() was given. Past the bank's size the entries hold +Inf and -1. exclude_self=True is for
        queries that ARE the bank (features = knn.bank_features, row m = bank row m): a row is then not its own neighbour."""
        m, dev, step = self._queries(features, chunk, "kneighbors", bool(exclude_self))
        d = torch.empty(m, self.k, dtype=torch.float32, device=dev)
        idx = torch.empty(m, self.k, dtype=torch.int64, device=dev)
        if m == 0:
            return d, idx
        q = _matrix(features, dev, "features")
        rows = torch.cat([self.bank_rows, torch.full((1,), -1, dtype=torch.int64, device=dev)])     # column -1 -> row -1
        for r0, dist, ws in self._chunks(q, m, step, dev):
            skip = torch.arange(r0, r0 + dist.shape[0], dtype=torch.int64, device=dev) if exclude_self else None
            d[r0:r0 + step], cols = N.ops().knn_topk(dist, self.k, skip, ws)
            idx[r0:r0 + step] = rows[cols]
        return d, idx

    def calibrate(self, tpr=0.95, chunk=None):
        """Sets knn.threshold (a 0-d fp32 device tensor) to the smallest leave-one-out unknown score s of the bank such that at least
        `tpr` of the bank rows score <= s: every bank row is scored against the bank without itself. Returns self."""
        if isinstance(tpr, bool) or not isinstance(tpr, (int, float)):
            raise TypeError(f"tpr must be a number, got {type(tpr).__name__}")
        if not 0.0 < tpr <= 1.0:
            raise ValueError(f"tpr must lie in (0, 1], got {tpr}")
        self._require_fit("calibrate")
        m, dev, step = self._queries(self.bank_features, chunk, "calibrate")
        scores = self._kth_overall(self.bank_features, m, step, dev, True)
        self.threshold = torch.sort(scores).values[max(1, math.ceil(tpr * m)) - 1].clone()
        return self

    # -------------------------------------------------------------------------------------------------------------- state
    def _restore(self, sd, tensors):
        """The threshold of the state dict is a 0-d tensor, or None before `calibrate`."""
        KNN.__init__(self, int(sd["k"]), sd["distance"], float(sd["bank_fraction"]), int(sd["seed"]))
        if tensors["bank_features"].dim() != 2:
            raise ValueError(f"state dict: bank_features must be [N, F], got shape {tuple(tensors['bank_features'].shape)}")
        n = tensors["bank_features"].shape[0]
        for k in ("bank_rows", "bank_labels"):
            if tuple(tensors[k].shape) != (n,):
                raise ValueError(f"state dict: {k} must hold one entry per bank row ({n}), got shape {tuple(tensors[k].shape)}")
        start = tensors["bank_start"]
        if start.dim() != 1 or start.numel() < 2 or int(start[0]) != 0 or int(start[-1]) != n or bool((start[1:] < start[:-1]).any()):
            raise ValueError(f"state dict: bank_start must be [C + 1] offsets rising from 0 to {n}, got {start.tolist()}")
        threshold = tensors["threshold"]
        if threshold is not None and threshold.dim() != 0:
            raise ValueError(f"state dict: threshold must be a scalar or None, got shape {tuple(threshold.shape)}")

"""ViM (Wang, Li, Feng, Zhang, "ViM: Out-Of-Distribution with Virtual-logit Matching", CVPR 2022) on the MI355X: the norm of a
feature's residual outside the principal subspace of the training features, scaled to the logits and matched against them as one
more, virtual, logit.

    vim = ViM(dim=None, origin="logit")
    vim.fit(features, logits, gt)                # the arrays of train.get_arrays on the TRAINING split; rows with gt < 0 are ignored
    n = vim.residual_norm(features)              # [M] fp32 on the device: |R (x - o)|, R the eigenvectors past the first `dim`
    unknown = vim.unknown_score(features, logits)        # [M]: alpha n - logsumexp(logits) (larger = more unknown)
    probs = vim.probabilities(features, logits)  # [M, C + 1]: softmax of [logits, alpha n], the virtual class last
    scores = vim.predict(features, logits)       # [M, C]: the first C columns of it

`fit` takes the second moment S = sum (x - o)(x - o)^T over the counted rows (osi_maha_scatter), its eigenvectors (`eigh`, below), keeps
all of them as `components [F, F]` (rows, by descending `eigenvalues [F]` of S) and sets alpha = sum max_c logits / sum n over the counted
rows, so that the virtual logit has the scale of the largest real one. The origin o is, with origin="logit", the point the last layer
maps to zero logits: o = -pinv(weight) bias for the layer's `weight [C, F]` and `bias [C]` (zero without a bias); that pinv is a one-off
C x F solve in fp64 numpy on the host, the only host arithmetic of this module. `origin` may also be an explicit [F] vector. `dim`
defaults to the paper's rule: 1000 for F >= 2048, 512 for F >= 768, else F // 2; 0 < dim < F.

`eigh(S)` is the symmetric eigensolver the fit runs on: parallel cyclic Jacobi in fp64 (csrc/vim.hip, torch.ops.osi.eigh_*),
deterministic and free of atomics, for F <= 4096. The loop is here: one sweep per call, one read-back per sweep (the number of
rotations), until a sweep rotates nothing; a solve that has not converged after `max_sweeps` raises ValueError. The method is not
part of the reference snapshot: include/osi.h (ABI 26) is its definition, tests/vim_oracle.py its numpy restatement.

Everything runs in fp64 in the kernels of csrc/vim.hip, the projection on the fp64 matrix cores; there is no CPU path. Inputs may be
numpy arrays or torch tensors, on the host or on the device. The fitted tensors are fp64 device tensors the caller may read. Rows go
through the kernels in the chunks of _detector._chunk_rows, or of `chunk=` rows. Out of scope: per-class subspaces, F > 4096, multi-GPU fits."""
import numpy as np
import torch

from . import _native as N
from ._detector import _MAX_ELEMS, Detector, _check_chunk, _chunk_rows, _fit_shapes, _matrix
from .util import _labels_on_device, _need_gpu


def default_dim(f_dim):
    """The paper's principal dimension for features of width F."""
    return 1000 if f_dim >= 2048 else 512 if f_dim >= 768 else f_dim // 2


def eigh(S, max_sweeps=30):
    """(values [F] descending, vectors [F, F] with the eigenvectors as ROWS, sweeps run) of the symmetric fp64 matrix S [F, F], on the
    device. Every row of `vectors` is signed so that its entry of largest magnitude is positive. Only symmetric input makes sense;
    symmetry is not checked. ValueError on a matrix that holds a NaN or an Inf, and when `max_sweeps` sweeps did not converge."""
    shape = tuple(torch.as_tensor(S).shape)
    if len(shape) != 2 or shape[0] != shape[1] or shape[0] == 0:
        raise ValueError(f"S must be a square matrix [F, F], got shape {shape}")
    if shape[0] > N.EIGH_MAX_F:
        raise ValueError(f"S is {shape[0]} columns wide; the eigensolver takes at most {N.EIGH_MAX_F}")
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, int) or max_sweeps < 1:
        raise ValueError(f"max_sweeps must be a positive int, got {max_sweeps!r}")
    dev = _need_gpu("eigh")
    s = torch.as_tensor(S).detach().to(device=dev, dtype=torch.float64).contiguous()
    ws = torch.empty(N.lib().osi_vim_workspace(1, 1, shape[0]), dtype=torch.uint8, device=dev)
    ops = N.ops()
    a, vt, head, info = ops.eigh_begin(s, ws)
    if int(info.item()) != 0:
        raise ValueError("eigh: the Frobenius norm of S is not finite (S holds a NaN or an Inf, or its squares overflow)")
    for sweep in range(1, max_sweeps + 1):
        if int(ops.eigh_sweep(a, vt, head, info, ws).item()) == 0:      # the one read-back of a sweep
            break
    else:
        raise ValueError(f"eigh: not converged after {max_sweeps} sweeps of a {shape[0]} x {shape[0]} matrix")
    values, vectors = ops.eigh_finish(a, vt, info, ws)
    return values, vectors, sweep


class ViM(Detector):
    _STATE = ("origin", "eigenvalues", "components")
    _SETTINGS = ("dim", "alpha", "count", "classes")    # what the fit found, not what the constructor takes
    _DTYPES = dict.fromkeys(_STATE, torch.float64)
    _FIT = "fit(features, logits)"
    max_sweeps = 30             # of the eigensolver in fit

    def __init__(self, dim=None, origin="logit"):
        if dim is not None:
            if isinstance(dim, bool) or not isinstance(dim, int):
                raise TypeError(f"dim must be an int or None, got {type(dim).__name__}")
            if dim < 1:
                raise ValueError(f"dim must be positive, got {dim}")
        if isinstance(origin, str):
            if origin != "logit":
                raise ValueError(f"origin must be 'logit' or a vector [F], got {origin!r}")
        else:
            if origin is None or isinstance(origin, (bool, int, float)):
                raise TypeError(f"origin must be 'logit' or a vector [F], got {type(origin).__name__}")
            origin = torch.as_tensor(origin).detach().to(device="cpu", dtype=torch.float64).contiguous().clone()
            if origin.dim() != 1 or origin.numel() == 0:
                raise ValueError(f"origin must be 'logit' or a vector [F], got shape {tuple(origin.shape)}")
        self.requested_dim, self.requested_origin = dim, origin
        for name in self._STATE + self._SETTINGS:
            setattr(self, name, None)
        self.sweeps = None
        self._ws = None

    # ------------------------------------------------------------------------------------------------------------ helpers
    def _scratch(self, n, f, dev):
        """The workspace of a scatter over n rows, of the eigensolver and of the scoring calls."""
        lib = N.lib()
        return self._workspace(max(lib.osi_maha_workspace(n, 1, f), lib.osi_vim_workspace(1, 1, f)), dev)

    def _origin_of(self, f_dim, c, weight, bias):
        """The origin [F] as a host fp64 tensor: the explicit one, or -pinv(weight) bias (fp64 numpy, the one host solve)."""
        if not isinstance(self.requested_origin, str):
            if self.requested_origin.numel() != f_dim:
                raise ValueError(f"origin holds {self.requested_origin.numel()} values, the features are {f_dim} columns wide")
            return self.requested_origin.clone()
        if bias is None:
            return torch.zeros(f_dim, dtype=torch.float64)
        if weight is None:
            raise ValueError("weight is needed with a bias: the origin is -pinv(weight) bias")
        host = lambda t: (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)
        w, b = host(weight), host(bias)
        if w.shape != (c, f_dim):
            raise ValueError(f"weight must be [{c}, {f_dim}] (classes, columns), got shape {w.shape}")
        if b.shape != (c,):
            raise ValueError(f"bias must be [{c}], got shape {b.shape}")
        if not (np.isfinite(w).all() and np.isfinite(b).all()):
            raise ValueError("weight and bias must be finite")
        return torch.from_numpy(-np.linalg.pinv(w) @ b)

    # ---------------------------------------------------------------------------------------------------------------- fit
    def fit(self, features, logits, gt=None, weight=None, bias=None, chunk=None):
        """Origin, second moment, its eigenvectors and alpha from features [N, F] and logits [N, C] of the training split; rows with
        gt < 0 are ignored (gt=None counts every row). `weight [C, F]` / `bias [C]`: the last layer, for origin="logit"; the origin is
        -pinv(weight) bias, computed once in fp64 numpy on the host (a C x F solve), and zero without a bias. `chunk`: rows per
        launch. Returns self."""
        f_shape, l_shape = _fit_shapes(features, gt, logits, gt_optional=True)
        rows, f_dim, c = f_shape[0], f_shape[1], l_shape[1]
        if f_dim > N.EIGH_MAX_F:
            raise ValueError(f"features are {f_dim} columns wide; the eigensolver takes at most {N.EIGH_MAX_F}")
        dim = default_dim(f_dim) if self.requested_dim is None else self.requested_dim
        if not 0 < dim < f_dim:
            raise ValueError(f"dim must satisfy 0 < dim < F, got dim {dim} for F = {f_dim}")
        _check_chunk(chunk)
        origin = self._origin_of(f_dim, c, weight, bias)
        dev = _need_gpu("ViM.fit")
        x, lg = _matrix(features, dev, "features"), _matrix(logits, dev, "logits")
        if gt is None:
            y = torch.zeros(rows, dtype=torch.int64, device=dev)
        else:
            y = _labels_on_device(gt, dev)
            if y.dim() != 1:
                raise ValueError(f"gt must be a vector [N_samples], got shape {tuple(y.shape)}")
            y = torch.where(y >= 0, 0, -1)                  # one class: the counted rows
        counted = y >= 0
        origin = origin.to(dev)
        mean = torch.stack([torch.zeros_like(origin), origin])          # [anything; origin]: OSI_MAHA_TOTAL reads row C = 1
        step = min((_MAX_ELEMS - 1) // f_dim, chunk or rows)
        ws = self._scratch(min(step, rows), f_dim, dev)
        ops = N.ops()
        s = torch.empty(f_dim, f_dim, dtype=torch.float64, device=dev)
        for r0 in range(0, rows, step):
            ops.maha_scatter(x[r0:r0 + step], y[r0:r0 + step], mean, N.MAHA_TOTAL, r0 > 0, s, ws)
        try:
            values, vectors, sweeps = eigh(s, self.max_sweeps)
        except ValueError as e:
            raise ValueError(f"ViM.fit: the second moment of the features has no eigen-decomposition ({e})") from None
        residual = vectors[dim:]                            # rows dim .. F - 1, contiguous
        step = min(_chunk_rows(max(f_dim, c + 1)), chunk or rows)
        sum_n = torch.zeros((), dtype=torch.float64, device=dev)
        sum_max = torch.zeros((), dtype=torch.float64, device=dev)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for r0 in range(0, rows, step):
            keep = counted[r0:r0 + step]
            n = ops.vim_scores(ops.vim_project(x[r0:r0 + step], origin, residual, ws), None, 0.0, N.VIM_NORM, True, ws)
            sum_n += torch.where(keep, n, zero).sum()
            sum_max += torch.where(keep, lg[r0:r0 + step].max(dim=1).values.double(), zero).sum()
        count, total_n, total_max = int(counted.sum().item()), float(sum_n.item()), float(sum_max.item())
        if count == 0:
            raise ValueError("gt holds no counted row (every label is negative)")
        alpha = total_max / total_n if total_n > 0 else float("nan")
        if not np.isfinite(alpha):
            raise ValueError(f"ViM.fit: alpha = sum of the largest logits / sum of the residual norms = {total_max} / {total_n} is not finite")
        self.origin, self.eigenvalues, self.components = origin, values, vectors
        self.dim, self.alpha, self.count, self.classes, self.sweeps = dim, alpha, count, c, sweeps
        return self

    # ------------------------------------------------------------------------------------------------------------ scoring
    def _score(self, features, logits, chunk, what, mode):
        self._require_fit(what)
        f_dim = self.components.shape[0]
        f_shape = tuple(torch.as_tensor(features).shape)
        if len(f_shape) != 2 or f_shape[1] != f_dim:
            raise ValueError(f"features must be [M, {f_dim}] (the width fit saw), got shape {f_shape}")
        if mode != N.VIM_NORM:
            l_shape = tuple(torch.as_tensor(logits).shape)
            if l_shape != (f_shape[0], self.classes):
                raise ValueError(f"logits must be [{f_shape[0]}, {self.classes}] (the rows of features, the classes fit saw), got shape {l_shape}")
        _check_chunk(chunk)
        dev = _need_gpu(f"ViM.{what}")
        self._on(dev)
        m = f_shape[0]
        out = torch.empty((m, self.classes + 1) if mode == N.VIM_PROBS else (m,), dtype=torch.float32, device=dev)
        if m == 0:
            return out
        q = _matrix(features, dev, "features")
        lg = None if mode == N.VIM_NORM else _matrix(logits, dev, "logits")
        step = min(_chunk_rows(max(f_dim, self.classes + 1)), chunk or m)
        ws = self._scratch(1, f_dim, dev)
        ops = N.ops()
        residual = self.components[self.dim:]
        for r0 in range(0, m, step):
            z = ops.vim_project(q[r0:r0 + step], self.origin, residual, ws)
            out[r0:r0 + step] = ops.vim_scores(z, None if lg is None else lg[r0:r0 + step], self.alpha, mode, False, ws)
        return out

    def residual_norm(self, features, chunk=None):
        """[M] fp32 on the device: the norm of (x - origin) projected onto the eigenvectors past the first `dim`."""
        return self._score(features, None, chunk, "residual_norm", N.VIM_NORM)

    def unknown_score(self, features, logits, chunk=None):
        """[M] fp32 on the device: alpha * residual norm - logsumexp(logits) (larger = more unknown)."""
        return self._score(features, logits, chunk, "unknown_score", N.VIM_UNKNOWN)

    def probabilities(self, features, logits, chunk=None):
        """[M, C + 1] fp32 on the device: the softmax of the logits with the virtual logit alpha * residual norm as the last column."""
        return self._score(features, logits, chunk, "probabilities", N.VIM_PROBS)

    def predict(self, features, logits, chunk=None):
        """[M, C] fp32: the known classes' columns of `probabilities` (larger = more known)."""
        return self._score(features, logits, chunk, "predict", N.VIM_PROBS)[:, :self.classes]

    # -------------------------------------------------------------------------------------------------------------- state
    def _restore(self, sd, t):
        if t["components"].dim() != 2 or t["components"].shape[0] != t["components"].shape[1]:
            raise ValueError(f"state dict: components must be [F, F], got shape {tuple(t['components'].shape)}")
        f_dim = t["components"].shape[0]
        for k in ("origin", "eigenvalues"):
            if tuple(t[k].shape) != (f_dim,):
                raise ValueError(f"state dict: {k} must have shape {(f_dim,)}, got {tuple(t[k].shape)}")
        dim, alpha, count, classes = int(sd["dim"]), float(sd["alpha"]), int(sd["count"]), int(sd["classes"])
        if not 0 < dim < f_dim:
            raise ValueError(f"state dict: dim must satisfy 0 < dim < F, got dim {dim} for F = {f_dim}")
        if not np.isfinite(alpha):
            raise ValueError(f"state dict: alpha must be finite, got {alpha}")
        if classes < 1:
            raise ValueError(f"state dict: classes must be positive, got {classes}")
        ViM.__init__(self, dim, t["origin"])
        self.dim, self.alpha, self.count, self.classes = dim, alpha, count, classes

"""The Mahalanobis detector (Lee, Lee, Lee, Shin, "A Simple Unified Framework for Detecting Out-of-Distribution Samples and
Adversarial Attacks", NeurIPS 2018) and its Relative variant (Ren et al., "A Simple Fix to Mahalanobis Distance for Improving Near-OOD
Detection", 2021) on the MI355X: class-conditional Gaussians with one tied covariance, on the features of a trained network.

    maha = Mahalanobis(shrinkage=0.0, relative=False)
    maha.fit(features, gt)                   # the arrays of train.get_arrays on the TRAINING split; classes = 0 .. max known label
    d2 = maha.distances(features)            # [M, C] fp32 on the device: squared Mahalanobis distances (relative: d2_c - d2_0)
    scores = maha.predict(features)          # [M, C] in (0, 1]: exp(-d2 / 2F), relative: 1 / (1 + exp(d2 / 2F)); larger = more known
    unknown = maha.unknown_score(features)   # [M]: the row minimum of distances (larger = more unknown)

`fit` takes the class means, the within-class scatter S over the n counted rows (rows with a label below 0 are ignored), factors
Sigma = (1 - shrinkage) S / n + shrinkage (tr S / n F) I = L L^T - the maximum-likelihood estimate of Lee et al., optionally shrunk
towards a scaled identity - and keeps W = L^-1 and the whitened means W mu_c; a distance is then |W x - W mu_c|^2. With
`relative=True` a background Gaussian (the mean of all counted rows, their total scatter, its own L0 and W0) is fitted too and its
distance subtracted. Sigma must be positive definite: with n - C < F and shrinkage = 0 it never is, and `fit` raises ValueError
naming the failed pivot. The method is not part of the reference snapshot: include/osi.h (ABI 25) is its definition,
tests/mahalanobis_oracle.py its numpy restatement.

Everything runs in fp64 in the kernels of csrc/mahalanobis.hip (torch.ops.osi.maha_*), the products on the fp64 matrix cores; there
is no CPU path. Inputs may be numpy arrays or torch tensors, on the host or on the device. `fit` reads back the number of classes
and the factorisation's status, the scoring calls read nothing back. The fitted state - `means [C + 1, F]` (row C the background mean),
`counts [C + 1]`, `L`, `W` `[F, F]`, `logdet [1]`, `whitened_means [C, F]` and, when relative, `L0`, `W0`, `logdet0`,
`whitened_mean0 [1, F]` - are fp64 device tensors the caller may read. Rows go through the kernels in chunks: scoring in the chunks of
_detector._chunk_rows (the fp64 whitened rows of a chunk are twice its size), fit in chunks under the ABI's limit of 2^31 elements per
matrix (a million rows at F = 2048; past it the scatter accumulates over the chunks and the means are put together from the chunks'
means and counts). Out of scope: per-class covariances, low-rank variants, input pre-processing, multi-GPU fits."""
import torch

from . import _native as N
from ._detector import _MAX_ELEMS, Detector, _check_chunk, _chunk_rows, _fit_shapes, _matrix
from .util import _labels_on_device, _need_gpu


class Mahalanobis(Detector):
    _STATE = ("means", "counts", "L", "W", "logdet", "whitened_means")
    _OPTIONAL = ("L0", "W0", "logdet0", "whitened_mean0")                   # the background Gaussian of relative=True
    _SETTINGS = ("shrinkage", "relative")
    _DTYPES = dict({k: torch.float64 for k in _STATE + _OPTIONAL}, counts=torch.int64)

    def __init__(self, shrinkage=0.0, relative=False):
        if isinstance(shrinkage, bool) or not isinstance(shrinkage, (int, float)):
            raise TypeError(f"shrinkage must be a number, got {type(shrinkage).__name__}")
        if not 0.0 <= shrinkage <= 1.0:                     # false for a NaN
            raise ValueError(f"shrinkage must lie in [0, 1], got {shrinkage}")
        if not isinstance(relative, bool):
            raise TypeError(f"relative must be a bool, got {type(relative).__name__}")
        self.shrinkage, self.relative = float(shrinkage), relative
        for name in self._STATE + self._OPTIONAL:
            setattr(self, name, None)
        self._ws = None

    # ---------------------------------------------------------------------------------------------------------------- fit
    def _factor(self, s, n, ws, what):
        lo, w, logdet, info = N.ops().maha_factor(s, 1.0 / n, self.shrinkage, ws)
        pivot = int(info.item())                            # the one status read of a fit
        if pivot != 0:
            raise ValueError(f"Mahalanobis.fit: the {what} covariance is not positive definite (pivot {pivot} of {s.shape[0]} failed; "
                             f"{n} counted rows, shrinkage {self.shrinkage}): pass a positive shrinkage")
        return lo, w, logdet

    def fit(self, features, gt, chunk=None):
        """Means, tied covariance, its Cholesky factor and inverse and the whitened means from features [N, F] and labels [N] of the
        training split; C = max(gt) + 1, rows with a negative label are ignored. `chunk`: rows per scatter launch. Returns self."""
        f_shape = _fit_shapes(features, gt)
        if f_shape[1] > N.MAHA_MAX_F:
            raise ValueError(f"features are {f_shape[1]} columns wide; the kernels take at most {N.MAHA_MAX_F}")
        _check_chunk(chunk)
        dev = _need_gpu("Mahalanobis.fit")
        y = _labels_on_device(gt, dev)
        if y.dim() != 1:
            raise ValueError(f"gt must be a vector [N_samples], got shape {tuple(y.shape)}")
        c = int(y.max().item()) + 1
        if c < 1:
            raise ValueError("gt holds no known class (every label is negative)")
        x = _matrix(features, dev, "features")
        rows, f_dim = x.shape
        step = min((_MAX_ELEMS - 1) // f_dim, chunk or rows)                # fit writes nothing per row: only the ABI's limit cuts it
        ws = self._workspace(N.lib().osi_maha_workspace(min(step, rows), c, f_dim), dev)
        ops = N.ops()
        if step >= rows:
            means, counts = ops.maha_class_means(x, y, c, ws)
        else:                                               # per-chunk sums (mean * count is the rounded sum), one division at the end
            sums = torch.zeros(c + 1, f_dim, dtype=torch.float64, device=dev)
            counts = torch.zeros(c + 1, dtype=torch.int64, device=dev)
            for r0 in range(0, rows, step):
                m, k = ops.maha_class_means(x[r0:r0 + step], y[r0:r0 + step], c, ws)
                sums += m * k[:, None].double()
                counts += k
            means = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None].double(), torch.zeros_like(sums))
        n = int(counts[c].item())
        modes = [(N.MAHA_WITHIN, "within-class")] + ([(N.MAHA_TOTAL, "total")] if self.relative else [])
        fitted = []
        for mode, what in modes:
            s = torch.empty(f_dim, f_dim, dtype=torch.float64, device=dev)
            for r0 in range(0, rows, step):
                ops.maha_scatter(x[r0:r0 + step], y[r0:r0 + step], means, mode, r0 > 0, s, ws)
            fitted.append(self._factor(s, n, ws, what))
        self.means, self.counts = means, counts
        self.L, self.W, self.logdet = fitted[0]
        self.whitened_means = ops.maha_whiten(means[:c].contiguous(), self.W, ws)
        if self.relative:
            self.L0, self.W0, self.logdet0 = fitted[1]
            self.whitened_mean0 = ops.maha_whiten(means[c:].contiguous(), self.W0, ws)
        else:
            self.L0 = self.W0 = self.logdet0 = self.whitened_mean0 = None
        return self

    # ------------------------------------------------------------------------------------------------------------ scoring
    def _score(self, features, chunk, what, transform):
        self._require_fit(what)
        f_shape = tuple(torch.as_tensor(features).shape)
        c, f_dim = self.whitened_means.shape
        if len(f_shape) != 2 or f_shape[1] != f_dim:
            raise ValueError(f"features must be [M, {f_dim}] (the width fit saw), got shape {f_shape}")
        _check_chunk(chunk)
        dev = _need_gpu(f"Mahalanobis.{what}")
        self._on(dev)
        m = f_shape[0]
        out = torch.empty(m, c, dtype=torch.float32, device=dev)
        if m == 0:
            return out
        q = _matrix(features, dev, "features")
        step = min(_chunk_rows(max(f_dim, c)), chunk or m)
        ws = self._workspace(N.lib().osi_maha_workspace(1, c, f_dim), dev)
        ops = N.ops()
        for r0 in range(0, m, step):
            rows = q[r0:r0 + step]
            minus = None
            if self.relative:
                minus = ops.maha_sqdist(ops.maha_whiten(rows, self.W0, ws), self.whitened_mean0, None, N.MAHA_RAW, True, ws).reshape(-1)
            out[r0:r0 + step] = ops.maha_sqdist(ops.maha_whiten(rows, self.W, ws), self.whitened_means, minus, transform, False, ws)
        return out

    def distances(self, features, chunk=None):
        """[M, C] fp32 on the device: squared Mahalanobis distances to the class means; with relative=True minus the squared distance
        under the background Gaussian (may be negative). `chunk`: rows per launch (default: as many as the ABI's limit allows)."""
        return self._score(features, chunk, "distances", N.MAHA_RAW)

    def predict(self, features, chunk=None):
        """[M, C] fp32 in (0, 1], larger = more known: exp(-d2 / 2F), with relative=True 1 / (1 + exp(d2 / 2F))."""
        return self._score(features, chunk, "predict", N.MAHA_SIM_LOGISTIC if self.relative else N.MAHA_SIM_GAUSS)

    def unknown_score(self, features, chunk=None):
        """[M] fp32 on the device: the smallest entry of the row of `distances` (larger = more unknown)."""
        return self._score(features, chunk, "unknown_score", N.MAHA_RAW).min(dim=1).values

    # -------------------------------------------------------------------------------------------------------------- state
    def _restore(self, sd, t):
        """The background entries of the state dict are None when not relative, and are not read then."""
        Mahalanobis.__init__(self, float(sd["shrinkage"]), bool(sd["relative"]))
        names = self._STATE
        if self.relative:
            names += self._OPTIONAL
            absent = [k for k in self._OPTIONAL if t[k] is None]
            if absent:
                raise ValueError(f"state dict holds no tensor for {absent}")
        else:
            t.update(dict.fromkeys(self._OPTIONAL))
        if t["whitened_means"].dim() != 2:
            raise ValueError(f"state dict: whitened_means must be [C, F], got shape {tuple(t['whitened_means'].shape)}")
        c, f_dim = t["whitened_means"].shape
        shapes = dict(means=(c + 1, f_dim), counts=(c + 1,), L=(f_dim, f_dim), W=(f_dim, f_dim), logdet=(1,), L0=(f_dim, f_dim),
                      W0=(f_dim, f_dim), logdet0=(1,), whitened_mean0=(1, f_dim))
        for k in names:
            if k in shapes and tuple(t[k].shape) != shapes[k]:
                raise ValueError(f"state dict: {k} must have shape {shapes[k]}, got {tuple(t[k].shape)}")

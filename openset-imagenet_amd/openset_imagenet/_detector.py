"""What the post-hoc open-set detectors (openmax.OpenMax, evm.EVM, knn.KNN, mahalanobis.Mahalanobis, vim.ViM, shaping.ActivationShaping;
odin.ODIN takes the base class alone) share on the host: the
argument checks of their `fit` and scoring calls, the sizes of the row chunks their kernels take, and `Detector`, the base class that
holds the fitted tensors, the workspace and the state dict. None of it computes: every check here runs before `_need_gpu`, so a host
without a GPU still gets the ValueError of a bad argument."""
import numpy as np
import torch

_DESC_LIMIT = 1 << 31           # the kernels' buffer descriptors are 32-bit (include/osi.h)
_CHUNK_BYTES = 1 << 29          # distance matrices are produced in row chunks of at most this size
_MAX_ELEMS = 1 << 31            # a call takes fewer elements than this in each of its matrices (include/osi.h)


def _matrix(x, dev, name):
    """[rows, columns] fp32 on the device."""
    t = torch.as_tensor(x).detach()
    if t.dim() != 2:
        raise ValueError(f"{name} must be a matrix [N_samples, N_columns], got shape {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _chunk_rows(columns):
    """Rows of a [rows, columns] fp32 distance chunk: under the descriptor limit and under _CHUNK_BYTES."""
    return max(1, min(_CHUNK_BYTES, _DESC_LIMIT - 1) // (4 * columns))


def _launch_rows(m, f_dim):
    """Rows of the [m, f_dim] fp32 queries one launch takes: all of them while they stay under the descriptor limit."""
    return max(1, (_DESC_LIMIT - 1) // (4 * f_dim)) if m * f_dim * 4 >= _DESC_LIMIT else max(m, 1)


def _check_chunk(chunk):
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"chunk must be a positive int or None, got {chunk!r}")


def _host_labels(gt):
    """gt [N] as an int64 numpy vector that names at least one known class (the one readback of the labels)."""
    y = (gt.detach().cpu().numpy() if isinstance(gt, torch.Tensor) else np.asarray(gt)).astype(np.int64)
    if y.ndim != 1:
        raise ValueError(f"gt must be a vector [N_samples], got shape {y.shape}")
    if y.max() < 0:
        raise ValueError("gt holds no known class (every label is negative)")
    return y


def _fit_shapes(features, gt, logits=None, gt_optional=False):
    """The shape checks of a fit: features [N, F], gt [N] (may be None with gt_optional) and, where the method takes them, logits [N, C],
    none of them empty. Returns the shape of features, or the shapes of features and logits."""
    f_shape = tuple(torch.as_tensor(features).shape)
    if len(f_shape) != 2:
        raise ValueError(f"features must be a matrix [N_samples, N_columns], got shape {f_shape}")
    if logits is None:
        l_shape = None
    else:
        l_shape = tuple(torch.as_tensor(logits).shape)
        if len(l_shape) != 2 or l_shape[0] != f_shape[0]:
            raise ValueError(f"logits must be a matrix [N_samples, N_classes] that agrees with features on the number of samples "
                             f"({f_shape[0]}), got shape {l_shape}")
    if not (gt is None and gt_optional) and len(gt) != f_shape[0]:
        raise ValueError(f"features and gt disagree on the number of samples: {f_shape[0]}, {len(gt)}")
    if l_shape is None:
        if f_shape[0] == 0 or f_shape[1] == 0:
            raise ValueError(f"features must not be empty, got shape {f_shape}")
        return f_shape
    if f_shape[0] == 0 or f_shape[1] == 0 or l_shape[1] == 0:
        raise ValueError(f"features and logits must not be empty, got shapes {f_shape}, {l_shape}")
    return f_shape, l_shape


class Detector:
    """The fitted state of a detector. A subclass names, as class attributes,

      _STATE      the tensors a fit always leaves; they are set together, so the first one tells whether the detector is fitted
      _OPTIONAL   the tensors that may stay None (Mahalanobis' background Gaussian, KNN's threshold)
      _SETTINGS   the plain values a state dict carries beside the tensors
      _DTYPES     the dtype a state dict's entry is cast to on loading, for every name of _STATE and _OPTIONAL
      _FIT        how its fit is called, for the "before fit" message

    and sets all of those attributes to None, with `_ws`, in its __init__."""
    _STATE = _OPTIONAL = _SETTINGS = ()
    _DTYPES = {}
    _FIT = "fit(features, gt)"

    @property
    def is_fitted(self):
        return getattr(self, self._STATE[0]) is not None

    def _require_fit(self, what):
        if not self.is_fitted:
            raise ValueError(f"{type(self).__name__}.{what} before fit: call {self._FIT} or load_state_dict first")

    def _on(self, dev):
        """The fitted tensors on `dev` (a state dict loads on the host; the first computing call moves them)."""
        if getattr(self, self._STATE[0]).device != dev:
            for name in self._STATE + self._OPTIONAL:
                if getattr(self, name) is not None:
                    setattr(self, name, getattr(self, name).to(dev))

    def _workspace(self, need, dev):
        """`need` bytes of scratch on `dev`, kept between calls and only ever grown."""
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    def state_dict(self):
        """Plain CPU tensors (None for an optional one that is not set) and the settings; torch.save-able."""
        self._require_fit("state_dict")
        sd = {name: getattr(self, name) for name in self._STATE + self._OPTIONAL}
        sd = {name: None if t is None else t.detach().cpu().clone() for name, t in sd.items()}
        sd.update({k: getattr(self, k) for k in self._SETTINGS})
        return sd

    def load_state_dict(self, sd):
        missing = [k for k in self._STATE + self._OPTIONAL + self._SETTINGS if k not in sd]
        if missing:
            raise ValueError(f"state dict lacks {missing}")
        absent = [k for k in self._STATE if sd[k] is None]
        if absent:
            raise ValueError(f"state dict holds no tensor for {absent}")
        tensors = {k: None if sd[k] is None else torch.as_tensor(sd[k]).detach().to(self._DTYPES[k]).contiguous().clone()
                   for k in self._STATE + self._OPTIONAL}
        self._restore(sd, tensors)
        for k, t in tensors.items():
            setattr(self, k, t)
        return self

    def _restore(self, sd, tensors):
        """The part of load_state_dict that differs: run __init__ again with the settings of `sd` and check the shapes of `tensors`
        (cast already; an optional entry may be None, and may be set to None here)."""
        raise NotImplementedError

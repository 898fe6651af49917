"""What the GPU parity tests of the detectors share when they call the C ABI directly: guard-banded outputs, a poisoned workspace,
bit-preserving uploads, and the bit / ulp comparisons. A plain module, imported like the oracles."""
import numpy as np
import torch

GUARD = 256                                  # bytes = 64 floats, before and after every output
CANARY = 0xA5


class Out:
    """A device output with guard bands: `t` is the tensor the kernel writes, check() says whether the bands kept their canary."""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((GUARD + (n + 7) // 8 * 8 + GUARD,), CANARY, dtype=torch.uint8, device=dev)
        self.n = n
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(*shape)

    def check(self):
        return bool((self.raw[:GUARD] == CANARY).all()) and bool((self.raw[GUARD + self.n:] == CANARY).all())

    def np(self):
        return self.t.cpu().numpy()


def call(fn, *args):
    """One C-ABI call on the current stream: tensors and Outs as pointers, the status checked, the device synchronised."""
    from openset_imagenet import _native as NL
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else (a.t.data_ptr() if isinstance(a, Out) else a) for a in args]
    NL.check(fn(*conv, torch.cuda.current_stream().cuda_stream), fn.__name__)
    torch.cuda.synchronize()


def poisoned(nbytes, dev, fill=None):
    """A workspace whose contents no kernel may rely on: 0xFF in every byte unless the test asks for another fill."""
    return torch.full((nbytes,), 0xFF if fill is None else fill, dtype=torch.uint8, device=dev)


def on(dev, *arrays):
    """Device copies that keep the input's bits and dtype (None stays None), always as a list: unpack it, `*on(dev, a)` for one array
    too. A copy is made on the host first, so read-only and non-contiguous arrays are fine."""
    return [None if a is None else torch.tensor(np.asarray(a)).to(dev) for a in arrays]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_bits_nan(a, b):
    """Equal fp32 bit patterns, a NaN compared as a NaN (its payload is not part of the definition)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


def ulps(a, b):
    """Distance in fp32 ulps between two finite fp32 arrays (NaN must sit in the same places)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return int(np.abs(key(a[ok]) - key(b[ok])).max()) if ok.any() else 0


def ulp32(ref):
    """The fp32 spacing at |ref|, as fp64."""
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def twice(run):
    """The call's output, after a second call (fresh output, fresh workspace) gave the same bits."""
    first, second = run(), run()
    assert same_bits_nan(first, second), "two runs differ"
    return first

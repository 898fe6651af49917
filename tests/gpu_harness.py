"""What the GPU parity tests of the detectors share when they call the C ABI directly: guard-banded outputs, a poisoned workspace,
bit-preserving uploads, 0xFF-banded inputs, and the bit / ulp comparisons. A plain module, imported like the oracles."""
import numpy as np
import torch

GUARD = 256                                  # bytes = 64 floats, before and after every output
CANARY = 0xA5


def _band(band):
    assert band >= 0 and band % 256 == 0, "a band is a multiple of 256 bytes: the payload keeps the alignment torch gives"
    return int(band)


def _banded(n, lead, trail, band_byte, dev):
    """(raw, payload) bytes: `lead` and `trail` bytes of `band_byte` around n payload bytes (padded to 8, the padding is band)."""
    raw = torch.full((lead + (n + 7) // 8 * 8 + trail,), band_byte, dtype=torch.uint8, device=dev)
    return raw, raw[lead:lead + n]


def _bands_hold(raw, lead, n, band_byte):
    return bool((raw[:lead] == band_byte).all()) and bool((raw[lead + n:] == band_byte).all())


class Out:
    """A device output with guard bands: `t` is the tensor the kernel writes, check() says whether the bands kept their canary.
    band: bytes before and after (a multiple of 256), or a pair (before, after). fill: the payload's pre-fill (NaN shows an unwritten
    float element in any comparison); None leaves the canary in it."""

    def __init__(self, shape, dtype, dev, band=GUARD, fill=None):
        self.lead, self.trail = (_band(b) for b in (band if isinstance(band, tuple) else (band, band)))
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw, payload = _banded(n, self.lead, self.trail, CANARY, dev)
        self.n = n
        self.t = payload.view(dtype).view(*shape)
        if fill is not None:
            self.t.fill_(fill)

    def check(self):
        return bool((self.raw[:self.lead] == CANARY).all()) and bool((self.raw[self.lead + self.n:] == CANARY).all())

    def np(self):
        return self.t.cpu().numpy()


class In:
    """A device copy of a CPU tensor (same bits) between bands of 0xFF bytes: a NaN in fp32 / fp64, -1 in an integer, 255 in a byte, so
    a load outside the tensor that reaches an accumulator shows as NaN in the output. `t` is the tensor to pass; unchanged() says
    that the payload still holds the uploaded bits and both bands are whole: the kernel wrote nothing into its input."""

    def __init__(self, tensor, dev, band=GUARD):
        self.lead = self.trail = _band(band)
        src = tensor.detach().cpu().contiguous()
        self.bits = src.reshape(-1).view(torch.uint8).clone()
        self.n = self.bits.numel()
        self.raw, payload = _banded(self.n, self.lead, self.trail, 0xFF, dev)
        payload.copy_(self.bits)
        self.t = payload.view(src.dtype).view(*src.shape)

    def unchanged(self):
        return _bands_hold(self.raw, self.lead, self.n, 0xFF) and torch.equal(self.raw[self.lead:self.lead + self.n].cpu(), self.bits)


class Ws:
    """A workspace of exactly nbytes between canary bands, every byte of it set to `fill`. nbytes = 0: ptr is None (a null pointer
    and size 0, as the header allows). check() as for Out."""

    def __init__(self, nbytes, dev, fill=0xFF, band=GUARD):
        self.lead = self.trail = _band(band)
        self.nbytes = self.n = int(nbytes)
        self.raw, self.t = _banded(self.n, self.lead, self.trail, CANARY, dev)
        self.t.fill_(fill)
        self.ptr = self.t.data_ptr() if self.n else None

    def check(self):
        return _bands_hold(self.raw, self.lead, self.n, CANARY)


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

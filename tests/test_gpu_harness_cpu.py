"""The detectors of tests/gpu_harness.py trip: every guarded GPU test rests on Out / In / Ws noticing one stray byte, and on 0xFF
bytes reading as NaN through a float view. On the CPU: the classes only need torch."""
import numpy as np
import pytest
import torch

import gpu_harness as H

NAN = float("nan")


def test_ff_bytes_are_nan_as_floats_and_minus_one_as_integers():
    raw = torch.full((64,), 0xFF, dtype=torch.uint8)
    assert bool(torch.isnan(raw.view(torch.float32)).all()) and bool(torch.isnan(raw.view(torch.float64)).all())
    assert bool((raw.view(torch.int32) == -1).all()) and bool((raw.view(torch.int64) == -1).all()) and bool((raw == 255).all())
    # one 0xFF byte in the exponent's place is not enough, which is why a band holds it in EVERY byte
    assert not bool(torch.isnan(torch.tensor([0, 0, 0, 0xFF], dtype=torch.uint8).view(torch.float32)).any())


@pytest.mark.parametrize("band", [256, (256, 1024), 0])
def test_out_bands_trip_on_one_byte(band):
    lead, trail = band if isinstance(band, tuple) else (band, band)
    o = H.Out((5, 3), torch.float32, "cpu", band=band, fill=NAN)
    assert o.t.shape == (5, 3) and o.t.data_ptr() == o.raw.data_ptr() + lead and o.raw.numel() == lead + 64 + trail
    assert bool(torch.isnan(o.t).all()) and o.check()
    o.t.fill_(1.0)                       # the payload is the kernel's to write
    assert o.check() and np.array_equal(o.np(), np.ones((5, 3), np.float32))
    if lead:
        o.raw[lead - 1] = 0
        assert not o.check()
        o.raw[lead - 1] = H.CANARY
        assert o.check()
    o.raw[lead + o.n] ^= 1               # the first byte behind the payload (60 bytes: the padding to 8 is band as well)
    assert not o.check()
    o.raw[lead + o.n] = H.CANARY
    if trail:
        o.raw[-1] = 0                    # and the far end of the trailing band
        assert not o.check()


def test_out_defaults_are_what_the_detector_tests_use():
    o = H.Out((4,), torch.int64, "cpu")
    assert o.raw.numel() == 2 * H.GUARD + 32 and bool((o.raw == H.CANARY).all()) and o.check()
    with pytest.raises(AssertionError):
        H.Out((4,), torch.float32, "cpu", band=100)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int64, torch.int32, torch.uint8])
def test_in_keeps_the_bits_and_trips_on_one_byte(dtype):
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 255, (7, 3), generator=g).to(dtype)
    if dtype.is_floating_point:
        src[0, 0], src[1, 1] = NAN, -0.0
    i = H.In(src.t(), "cpu")             # a non-contiguous source is copied in logical order
    assert i.t.dtype == dtype and i.t.shape == (3, 7) and H.same_bytes(i.t.numpy(), src.t().contiguous().numpy())
    assert i.t.data_ptr() % 16 == i.raw.data_ptr() % 16
    assert bool((i.raw[:i.lead] == 0xFF).all()) and bool((i.raw[i.lead + i.n:] == 0xFF).all()) and i.unchanged()
    halo = i.raw[:i.lead].view(dtype)
    assert bool(torch.isnan(halo).all()) if dtype.is_floating_point else bool((halo == (255 if dtype == torch.uint8 else -1)).all())
    for at in (0, i.lead - 1, i.lead + i.n, i.raw.numel() - 1):      # both ends of both bands
        i.raw[at] = 0xFE
        assert not i.unchanged()
        i.raw[at] = 0xFF
        assert i.unchanged()
    keep = int(i.raw[i.lead + 5])
    i.raw[i.lead + 5] = keep ^ 0x80      # one bit of one payload byte
    assert not i.unchanged()
    i.raw[i.lead + 5] = keep
    assert i.unchanged()


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_ws_is_exact_poisoned_and_trips_on_one_byte(fill):
    w = H.Ws(100, "cpu", fill=fill)
    assert w.nbytes == 100 and w.t.numel() == 100 and w.ptr == w.t.data_ptr() and bool((w.t == fill).all()) and w.check()
    w.t.fill_(7)                         # contents are the kernel's
    assert w.check()
    w.raw[w.lead - 1] = 0
    assert not w.check()
    w.raw[w.lead - 1] = H.CANARY
    w.raw[w.lead + 100] = 0              # byte 100 of a 100-byte workspace
    assert not w.check()


def test_ws_of_no_bytes_is_a_null_pointer():
    w = H.Ws(0, "cpu")
    assert w.ptr is None and w.nbytes == 0 and w.check()
    w.raw[w.lead] = 0                    # whatever is written through a zero-size workspace lands in a band
    assert not w.check()

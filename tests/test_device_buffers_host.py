"""Host: the guarded-buffer harness of the post-processing GPU tests (tests/_device_buffers.py) on CPU tensors.  The harness is what
tells those tests that a kernel wrote out of bounds or into an input, so each of its assertions is made to fire once here, by ordinary
tensor assignments."""
import numpy as np
import pytest
import torch

from tests._device_buffers import GUARD_BYTES, Guarded

DTYPES = [torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64]
SENTINEL = {torch.int32: -777, torch.int64: -777, torch.uint8: 0xA5, torch.float32: -777.0, torch.float64: -777.0}


def buffers(dtype, n=37):
    data = (np.arange(n) % 7 + 1).astype(np.float64)           # never the sentinel
    return Guarded(n, dtype, name="out", device="cpu"), Guarded(n, dtype, data, "in", device="cpu"), data


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_bands_are_4096_bytes_and_a_clean_buffer_passes(dtype):
    out, inp, data = buffers(dtype)
    size = torch.empty(0, dtype=dtype).element_size()
    assert GUARD_BYTES == 4096
    for g in (out, inp):
        assert g.g * size == 4096 and g.buf.numel() == 37 + 2 * 4096 // size and g.sent == SENTINEL[dtype]
        assert g.t.numel() == 37 and g.t.dtype == dtype and g.p == g.buf.data_ptr() + 4096
        assert bool((g.buf[:g.g] == g.sent).all()) and bool((g.buf[g.g + 37:] == g.sent).all())
        g.check()
    assert bool((out.t == out.sent).all()) and np.array_equal(inp.host(), data.astype(inp.host().dtype))
    assert inp.host((1, 37)).shape == (1, 37)
    empty = Guarded(0, dtype, np.zeros(0), "empty", device="cpu")   # an input without elements goes as NULL and still checks
    assert empty.p is None and empty.host().size == 0
    empty.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_check_sees_one_element_on_either_side_and_a_changed_input(dtype):
    for at, text in ((-1, "out: guard band BEFORE the buffer was written"), (37, "out: guard band AFTER the buffer was written")):
        out, _, _ = buffers(dtype)
        out.buf[out.g + at] = 1
        with pytest.raises(AssertionError, match=text):
            out.check()
        with pytest.raises(AssertionError, match="workspace: guard band"):
            out.check("workspace")
    _, inp, _ = buffers(dtype)
    inp.t[36] = 0
    with pytest.raises(AssertionError, match="in is an input"):
        inp.check()
    out, _, _ = buffers(dtype)
    out.t[:] = 3                                                # an output may hold anything
    out.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_all_written_wants_every_element(dtype):
    out, _, _ = buffers(dtype)
    out.t[:36] = 3
    with pytest.raises(AssertionError, match="out: not every element was written"):
        out.all_written()
    out.t[36] = 0
    out.all_written()


def test_nan_is_a_legal_input():
    g = Guarded(3, torch.float64, [1.0, float("nan"), -0.0], "xy", device="cpu")
    g.check()
    g.t[2] = 0.0                                                # compared as bytes: the sign of a zero counts
    with pytest.raises(AssertionError, match="xy is an input"):
        g.check()

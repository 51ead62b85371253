"""The guarded device buffers of the post-processing GPU tests (test_gpu_{instances,dbscan,match,rle,poly,idmap}.py): every buffer a
kernel is handed sits between two 4 KiB bands of a sentinel, outputs start as the sentinel, and after the call the bands must be intact
and the inputs unchanged.  Plain helpers, imported like the _*_reference.py modules; the 2-D NaN-filled Guarded of test_gpu_conv_exact.py
is a different thing and stays there."""
import numpy as np
import torch

GUARD_BYTES = 4096


class Guarded:
    """n elements between two guard bands; everything starts as the sentinel.  With `data` the buffer is an input."""

    def __init__(self, n, dtype, data=None, name=None, device="cuda"):
        self.n, self.name, self.g = n, name, GUARD_BYTES // torch.empty(0, dtype=dtype).element_size()
        self.sent = 0xA5 if dtype == torch.uint8 else -777.0 if dtype.is_floating_point else -777
        self.buf = torch.full((n + 2 * self.g,), self.sent, dtype=dtype, device=device)
        self.data = None
        if data is not None:
            self.data = torch.as_tensor(np.ascontiguousarray(data)).to(dtype).reshape(-1)
            assert self.data.numel() == n
            self.buf[self.g:self.g + n] = self.data.to(device)

    @property
    def t(self):
        return self.buf[self.g:self.g + self.n]

    @property
    def p(self):
        return self.t.data_ptr() if self.n else None          # an empty buffer goes through the C ABI as NULL

    def host(self, shape=-1):
        return self.t.cpu().numpy().reshape(shape)

    def check(self, what=None):
        what = self.name if what is None else what
        assert bool((self.buf[:self.g] == self.sent).all()), f"{what}: guard band BEFORE the buffer was written"
        assert bool((self.buf[self.g + self.n:] == self.sent).all()), f"{what}: guard band AFTER the buffer was written"
        if self.data is not None:                              # compared as bytes: NaN is a legal input
            assert self.host().tobytes() == self.data.numpy().tobytes(), f"{what} is an input"

    def all_written(self, what=None):
        assert not bool((self.t == self.sent).any()), f"{self.name if what is None else what}: not every element was written"


def call(name, *args):
    """One entry point through _lib.call on the current stream: Guarded arguments go as their pointers, everything else (None
    included) as it is; then synchronise and check() every Guarded that was passed."""
    from maskunet_amd import _lib
    _lib.call(name, *[a.p if isinstance(a, Guarded) else a for a in args], _lib.stream())
    torch.cuda.synchronize()
    for a in args:
        if isinstance(a, Guarded):
            a.check()


def side_of(inst):
    """an Instances as the dict of numpy arrays that the restatements return (`values` and `invalid` where the producer sets them)"""
    names = {"ids": "ids", "count": "count", "table": "table", "score": "scores", "order": "order", "values": "values", "invalid": "invalid"}
    return {k: getattr(inst, f).cpu().numpy() for k, f in names.items() if getattr(inst, f) is not None}

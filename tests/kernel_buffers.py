"""Buffers of the kernel-level GPU tests: the library handle with its error convention, and device
memory that a kernel writes between two guards of 0xA5 bytes, which must be intact afterwards."""
import numpy as np
import torch

POISON = 0xA5
GUARD = 64


class Lib:
    def __init__(self):
        from nvtabular_amd import _lib
        from nvtabular_amd import kernels as K

        self.m, self.lib, self.K = _lib, _lib.load(), K

    def call(self, name, *args):
        self.m.check(getattr(self.lib, name)(*args, self.K.stream_ptr()), name)

    def refused(self, name, *args, by=None):
        """The call returns NVT_EINVAL and leaves a message that names it (or the helper ``by`` that
        checks its arguments): nothing was launched."""
        assert getattr(self.lib, name)(*args, self.K.stream_ptr()) == -1, name         # NVT_EINVAL
        msg = self.lib.nvt_last_error()
        assert msg and (by or name).encode() in msg, msg
        return msg.decode()


class Guarded:
    """``nbytes`` of device memory filled with 0xA5 between two guards of ``guard`` bytes (a multiple
    of 64; the allocation is 256-byte aligned, so ``ptr`` is aligned to min(guard, 256))."""

    def __init__(self, nbytes, guard=GUARD, init=None):
        self.nbytes, self.guard = int(nbytes), guard
        self.raw = torch.full((self.nbytes + 2 * guard,), POISON, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0 and guard % 64 == 0
        if init is not None:
            b = np.ascontiguousarray(init).view(np.uint8).ravel()
            assert b.size == self.nbytes
            self.raw[guard: guard + self.nbytes] = torch.from_numpy(b.copy()).to("cuda")

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.guard

    def read(self, dtype=np.uint8, what=""):
        """The bytes between the guards (the copy waits for the launches on the current stream)."""
        h = self.raw.cpu().numpy()
        g = self.guard
        assert (h[:g] == POISON).all(), f"{what}: bytes in front of the buffer were written"
        assert (h[g + self.nbytes:] == POISON).all(), f"{what}: bytes behind the buffer were written"
        return h[g: g + self.nbytes].view(dtype)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def p_(t):
    return None if t is None else t.data_ptr()

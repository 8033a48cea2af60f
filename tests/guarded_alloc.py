"""Exact guard zones around device buffers (a helper module of the test suite: not a conftest.py, and pytest does not collect it).

GuardedAllocator.zeros() carves each buffer out of a larger uint8 allocation that holds 4 KB of 0xA5 directly in front of the
buffer's first byte and 4 KB directly behind its last byte: no round-up slack, so a write of ONE byte past either end of the buffer
is seen.  The buffer itself starts 16-byte aligned (plus an optional byte offset, which lets a test hand a kernel a deliberately
misaligned view).  check() raises an AssertionError that names every damaged buffer: its tag, shape, dtype and the first corrupted
offset on either side.

    alloc = GuardedAllocator()
    with alloc.patch():                 # torch.zeros / torch.zeros_like on the allocator's device type are guarded meanwhile
        env = VecEWN(...)
    ...launches...
    alloc.check()
"""
import contextlib
import math

import torch

GUARD = 4096
FILL = 0xA5
ALIGN = 16


class GuardedBuffer:
    """one guarded allocation: parent[start:start + nbytes] is the buffer, every other byte of parent is guard"""

    def __init__(self, parent, start, nbytes, shape, dtype, tag):
        self.parent, self.start, self.nbytes, self.shape, self.dtype, self.tag = parent, start, nbytes, shape, dtype, tag

    @property
    def view_start(self):
        return self.start

    @property
    def view_end(self):
        return self.start + self.nbytes

    def damage(self):
        """(front, back): None for an intact side, else (offset of the first corrupted byte counted from the buffer's edge, number of
        corrupted bytes).  Front offsets are negative (-1 = the byte just before the buffer), back offsets count from 0 (the byte
        just behind its last byte)."""
        front, back = self.parent[:self.start], self.parent[self.view_end:]
        out = []
        for side, g in (("front", front), ("back", back)):
            bad = g != FILL
            if not bool(bad.any()):
                out.append(None)
                continue
            idx = torch.nonzero(bad).reshape(-1)
            n = int(idx.numel())
            # the corrupted byte nearest the buffer: an overrun starts at the edge and runs outwards
            first = int(idx[-1]) - self.start if side == "front" else int(idx[0])
            out.append((first, n))
        return tuple(out)

    def describe(self):
        return "%s shape=%s dtype=%s (%d bytes)" % (self.tag, tuple(self.shape), self.dtype, self.nbytes)


class GuardedAllocator:
    def __init__(self, device_type="cuda", guard=GUARD):
        self.device_type, self.guard = device_type, int(guard)
        self.buffers = []
        self._real_zeros, self._real_zeros_like = torch.zeros, torch.zeros_like
        self.tag = "untagged"

    # -- allocation
    def zeros(self, shape, dtype=torch.float32, device=None, tag=None, offset=0):
        """a zero-filled tensor of `shape` / `dtype` with guards directly around it; `offset` bytes past a 16-byte boundary"""
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        device = torch.device(self.device_type if device is None else device)
        esize = torch.empty((), dtype=dtype).element_size()
        nbytes = math.prod(shape) * esize
        G = self.guard
        parent = torch.full((G + ALIGN + int(offset) + nbytes + G,), FILL, dtype=torch.uint8, device=device)
        start = G + (-(parent.data_ptr() + G)) % ALIGN + int(offset)
        parent[start:start + nbytes] = 0
        rec = GuardedBuffer(parent, start, nbytes, shape, dtype, self.tag if tag is None else tag)
        self.buffers.append(rec)
        return parent[start:start + nbytes].view(dtype).view(shape)

    def zeros_like(self, t, dtype=None, tag=None):
        return self.zeros(t.shape, dtype=t.dtype if dtype is None else dtype, device=t.device, tag=tag)

    def owns(self, t):
        """True if `t` starts at the first byte of one of this allocator's guarded buffers"""
        return self.record(t) is not None

    def record(self, t):
        p = t.data_ptr()
        for r in self.buffers:
            if r.parent.data_ptr() + r.start == p and r.parent.device == t.device:
                return r
        return None

    # -- torch.zeros / torch.zeros_like on this device type, guarded
    def _guarded_zeros(self, *size, dtype=None, device=None, **kw):
        if kw or device is None or torch.device(device).type != self.device_type:
            return self._real_zeros(*size, dtype=dtype, device=device, **kw)
        shape = size[0] if len(size) == 1 and not isinstance(size[0], int) else size
        return self.zeros(shape, dtype=torch.get_default_dtype() if dtype is None else dtype, device=device)

    def _guarded_zeros_like(self, t, dtype=None, device=None, **kw):
        dev = t.device if device is None else torch.device(device)
        if kw or dev.type != self.device_type:
            return self._real_zeros_like(t, dtype=dtype, device=device, **kw)
        return self.zeros(t.shape, dtype=t.dtype if dtype is None else dtype, device=dev)

    @contextlib.contextmanager
    def patch(self, tag="untagged"):
        """torch.zeros / torch.zeros_like hand out guarded buffers (tagged `tag`) while the block runs"""
        saved = self.tag
        self.tag = tag
        torch.zeros, torch.zeros_like = self._guarded_zeros, self._guarded_zeros_like
        try:
            yield self
        finally:
            torch.zeros, torch.zeros_like = self._real_zeros, self._real_zeros_like
            self.tag = saved

    # -- verification
    def check(self, context=""):
        problems = []
        for r in self.buffers:
            front, back = r.damage()
            if front is None and back is None:
                continue
            msg = r.describe()
            if front is not None:
                msg += "; front guard: first corrupted byte at %d (%d bytes)" % front
            if back is not None:
                msg += "; back guard: first corrupted byte at end+%d (%d bytes)" % back
            problems.append(msg)
        assert not problems, "write outside a guarded buffer%s:\n  %s" % ((" (%s)" % context) if context else "", "\n  ".join(problems))

    def clear(self):
        self.buffers.clear()

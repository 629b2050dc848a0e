"""Guarded buffers for the memory contract of include/mpcqp.h (test helper, pure torch, CPU or GPU).

An arena is ONE uint8 tensor carved into [guard | buffer | guard | buffer | ... | guard]:

* every buffer starts 512-byte aligned (what torch's allocator gives the host code of qpmpc_amd) and is exactly as long as asked
  -- the byte count the header or a *_workspace_bytes query names, never rounded up;
* every guard is at least 64 KiB (plus what the alignment of the next buffer needs) and holds one fixed byte.

A launch that stores past a buffer, or in front of it, lands in a guard and `guards_intact()` names the buffer and the distance; a
launch that reads past an operand reads the guard's byte. With the byte 0xFF that is a NaN in both float widths and -1 as an int32:
a stale or over-read VALUE poisons the result, a stale INDEX (at most 64 KiB / 8 elements back) still points into the arena."""
from __future__ import annotations

GUARD = 64 * 1024
ALIGN = 512
PATTERN = 0xA5


def _torch():
    import torch

    return torch


def capacity_for(sizes) -> int:
    """Bytes of an arena that holds buffers of these sizes (an upper bound: the alignment slack is counted in full)."""
    return ALIGN + GUARD + sum(int(s) + GUARD + ALIGN for s in sizes)


class Arena:
    def __init__(self, capacity: int, device="cpu", pattern: int = PATTERN):
        torch = _torch()
        self.mem = torch.empty((int(capacity),), dtype=torch.uint8, device=device)
        self.base = self.mem.data_ptr()
        self.pattern = int(pattern)
        self.mem.fill_(self.pattern)
        self.spans = {}     # name -> (offset, nbytes)
        self.views = {}     # name -> typed view
        self.order = []     # names by address
        self._end = 0       # end of the last buffer
        self._saved = {}

    # ------------------------------------------------------------------ carving
    def carve(self, name: str, nbytes: int, dtype=None):
        """(typed view, device pointer) of a new buffer of exactly `nbytes`, 512-byte aligned, a guard on either side."""
        torch = _torch()
        if name in self.spans:
            raise KeyError(f"{name} is carved already")
        dtype = dtype or torch.uint8
        esz = torch.empty((), dtype=dtype).element_size()
        nbytes = int(nbytes)
        if nbytes % esz:
            raise ValueError(f"{name}: {nbytes} bytes is no whole number of {dtype} elements")
        off = self._end + GUARD
        off += (-(self.base + off)) % ALIGN
        if off + nbytes + GUARD > self.mem.numel():
            raise MemoryError(f"arena of {self.mem.numel()} bytes is full at {name} ({nbytes} bytes)")
        self.spans[name] = (off, nbytes)
        self.order.append(name)
        self._end = off + nbytes
        view = self.mem[off:off + nbytes].view(dtype)
        self.views[name] = view
        return view, self.base + off

    def view(self, name):
        return self.views[name]

    def ptr(self, name) -> int:
        return self.base + self.spans[name][0]

    def nbytes(self, name) -> int:
        return self.spans[name][1]

    def raw(self, name):
        off, nb = self.spans[name]
        return self.mem[off:off + nb]

    # ------------------------------------------------------------------ fills
    def fill(self, names, byte: int) -> None:
        for name in names:
            self.raw(name).fill_(int(byte))

    def _guards(self):
        """(start, end, buffer before | None, buffer after | None) of every guard, by address."""
        out, at, before = [], 0, None
        for name in self.order:
            off, nb = self.spans[name]
            out.append((at, off, before, name))
            at, before = off + nb, name
        out.append((at, self.mem.numel(), before, None))
        return out

    def fill_guards(self, byte: int) -> None:
        self.pattern = int(byte)
        for lo, hi, _, _ in self._guards():
            self.mem[lo:hi].fill_(self.pattern)

    def guards_intact(self):
        """[] when every guard holds its byte; else one (buffer, side, first, last, count) per damaged side of a buffer: side
        "after" -- bytes first .. last PAST the buffer's end (0 = the byte right behind it) --, or "before" -- bytes first .. last
        in front of its start (1 = the byte right in front of it); count of them differ from the guard's byte. A guard between two
        buffers is split in the middle between them."""
        damaged = []
        for lo, hi, before, after in self._guards():
            bad = (self.mem[lo:hi] != self.pattern).nonzero().flatten()
            if bad.numel() == 0:
                continue
            bad = bad.cpu()
            mid = (hi - lo) // 2 if (before is not None and after is not None) else (hi - lo if after is None else 0)
            near, far = bad[bad < mid], bad[bad >= mid]
            if near.numel():
                damaged.append((before, "after", int(near.min()), int(near.max()), int(near.numel())))
            if far.numel():
                dist = (hi - lo) - far  # 1 = the byte right in front of the buffer
                damaged.append((after, "before", int(dist.min()), int(dist.max()), int(far.numel())))
        return damaged

    # ------------------------------------------------------------------ read-only buffers
    def snapshot(self, names) -> None:
        for name in names:
            self._saved[name] = self.raw(name).clone()

    def unchanged(self, names=None):
        """[] when every snapshotted buffer (of `names`) still holds its bytes; else (name, first byte offset, count)."""
        torch = _torch()
        changed = []
        for name in (self._saved if names is None else names):
            now, then = self.raw(name), self._saved[name]
            if not torch.equal(now, then):
                bad = (now != then).nonzero().flatten()
                changed.append((name, int(bad.min()), int(bad.numel())))
        return changed

"""Caller-owned device workspaces (the library never allocates device memory): the one place that allocates and aligns them.

A workspace of `nbytes` is a uint8 buffer of `nbytes + 256`; the library is handed the first 256-aligned address inside it,
so `aligned_ptr(buf) + nbytes` never passes the buffer's end, whatever address the allocator returned.
"""
from __future__ import annotations

import torch


def alloc(nbytes, device):
    return torch.empty(nbytes + 256, dtype=torch.uint8, device=device)


def aligned_ptr(buf):
    return (buf.data_ptr() + 255) & ~255


def holds(buf, nbytes):
    return buf is not None and buf.numel() >= nbytes + 256


class Scratch(dict):
    """Scratch that carries nothing between calls: one buffer per (device, stream, *extra), grown on demand.  Calls on one
    stream are ordered, so they share it.  The dict maps those keys to the live buffers."""

    def take(self, device, nbytes, *extra):
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream) + extra
        buf = self.get(key)
        if not holds(buf, nbytes):
            buf = self[key] = alloc(nbytes, device)
        return buf


class Carried(dict):
    """Workspaces that carry a forward's activations to its backward: one per forward in flight.  The forward takes one (a
    fresh buffer if none is free, or if the free one is too small), the backward gives it back.  A training step runs
    forward then backward, so the previous step's buffer is free again; a second forward before the first one's backward
    takes another.  At most `keep` free buffers are held per key (None: all of them).  The dict maps keys to free buffers."""

    def __init__(self, keep=None):
        super().__init__()
        self.keep = keep

    def take(self, key, device, nbytes):
        free = self.get(key)
        buf = free.pop() if free else None
        return buf if holds(buf, nbytes) else alloc(nbytes, device)

    def give(self, key, buf):
        free = self.setdefault(key, [])
        free.append(buf)             # (stream-ordered behind the backward that gives it)
        if self.keep is not None:
            del free[:-self.keep]

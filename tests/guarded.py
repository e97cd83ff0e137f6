"""A guarded allocator for tests: every workspace and every output of a node lies between two bands of test-owned bytes.

`guarded(fill)` replaces, while it is active and with plain set-and-restore (nothing in the package changes),

  * `neural_ode_features_amd.workspace.alloc`: the returned uint8 buffer starts at a 256-byte aligned address inside a
    larger allocation, so `aligned_ptr(buf) == buf.data_ptr()` and the library's legal range is exactly
    `[ptr, ptr + nbytes)`.  The buffer is `nbytes + 256` long as the package expects (`workspace.holds`), but its last
    256 bytes -- the slack `alloc` adds -- belong to the guard, like the band on each side;
  * `torch.empty` / `torch.empty_like` for contiguous tensors of the guarded device type: the body starts at a 256-byte
    aligned address of a larger allocation with a band on each side.  The tensor is built with
    `torch.empty(0, dtype=...).set_(storage, offset, shape)`: a real tensor, not a view, so an autograd Function may
    return it;
  * `torch.zeros` for the guarded device type: a zero body between bands of `fill`.

Body and bands are filled with the byte `fill` (0xFF: NaN in every float format; 0x7F: 3.39e38 in fp32, finite -- what
`fmaxf`, ReLU masks and argmax do not swallow; 0x00).  The context records every allocation; `check()` synchronises and
asserts that every band byte still equals `fill`, naming the allocation, the side and the offset of the first byte hit.

A band is max(1 MiB, body size) on each side: an overrun of a tile or a row lands in memory the test owns and shows up as
a failed assertion.

`embed(t, fill)` copies a test-made input (an activation, a cotangent, a parameter's `.data`, labels) into the middle of
such a banded allocation and returns the interior tensor; `Embedded.check()` asserts that neither the input nor its bands
changed.  An over-read of an input that reaches a result then changes that result from one fill to the next.

`Case`, `plain_run`, `guarded_run` and `verify` are the checks of one case, shared by tests/test_gpu_guard_bands.py (the nodes) and
tests/test_guarded_host.py (fake nodes with one fault each, on the CPU).  `spied` records what the library's own functions return
during a run, so that "the node ran" is read off the library: its entry points were called, and the workspace that was asked for has
exactly the size its `*_workspace_bytes` function returned to the wrapper.
"""
from __future__ import annotations

import contextlib

import torch

FILLS = (0xFF, 0x7F, 0x00)
MIN_BAND = 1 << 20
ALIGN = 256
SLACK = 256          # what workspace.alloc adds behind nbytes

# the originals, taken once at import: patch and restore always go between these objects and the wrappers
_REAL_EMPTY = torch.empty
_REAL_EMPTY_LIKE = torch.empty_like
_REAL_ZEROS = torch.zeros


def _band_bytes(body_bytes, band_bytes):
    band = max(int(band_bytes), int(body_bytes), ALIGN)
    return (band + ALIGN - 1) // ALIGN * ALIGN


class Region:
    """One banded allocation: `raw` = [pad][left band][body (+ guarded tail)][right band], all uint8."""

    def __init__(self, what, raw, start, body_bytes, tail_bytes, band, fill):
        self.what, self.raw, self.start, self.fill = what, raw, start, fill
        self.body_bytes, self.tail_bytes, self.band = body_bytes, tail_bytes, band

    def spans(self):
        s = self.start
        return (('left band', s - self.band, s, 0),                                       # offsets reported relative to the body's start
                ('slack behind nbytes', s + self.body_bytes, s + self.body_bytes + self.tail_bytes, self.body_bytes),
                ('right band', s + self.body_bytes + self.tail_bytes, s + self.body_bytes + self.tail_bytes + self.band, self.body_bytes))

    def damage(self):
        """None, or a sentence on the first guard byte that no longer equals `fill`."""
        for side, lo, hi, _ in self.spans():
            if hi == lo:
                continue
            bad = (self.raw[lo:hi] != self.fill).nonzero()
            if bad.numel():
                at = lo + int(bad[0])
                rel = at - self.start
                where = ('%d bytes before its start' % -rel) if rel < 0 else ('at byte offset %d (%d past its %d bytes)' % (rel, rel - self.body_bytes, self.body_bytes))
                return '%s: %s written, %d byte(s) changed, first %s, now 0x%02X, fill 0x%02X' % (
                    self.what, side, int(bad.numel()), where, int(self.raw[at]), self.fill)
        return None


def _region(what, body_bytes, tail_bytes, band_bytes, fill, device):
    band = _band_bytes(body_bytes + tail_bytes, band_bytes)
    total = ALIGN + 2 * band + body_bytes + tail_bytes
    raw = _REAL_EMPTY(total, dtype=torch.uint8, device=device)
    raw.fill_(fill)
    start = (-raw.data_ptr()) % ALIGN + band          # band is a multiple of ALIGN: the body starts 256-byte aligned
    return Region(what, raw, start, body_bytes, tail_bytes, band, fill)


def _interior(region, shape, dtype):
    """A real (non-view) tensor of `shape` on the body's bytes."""
    itemsize = _REAL_EMPTY(0, dtype=dtype).element_size()
    assert (region.raw.storage_offset() + region.start) % itemsize == 0
    t = _REAL_EMPTY(0, dtype=dtype, device=region.raw.device)
    t.set_(region.raw.untyped_storage(), (region.raw.storage_offset() + region.start) // itemsize, tuple(shape))
    assert t.data_ptr() % ALIGN == 0 and t.is_contiguous()
    return t


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _shape_of(args, kwargs):
    if 'size' in kwargs:
        shape = kwargs['size']
    elif len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        shape = args[0]
    else:
        shape = args
    if isinstance(shape, int):
        shape = (shape,)
    return tuple(int(s) for s in shape)


class Guard:
    def __init__(self, fill, band_bytes=MIN_BAND, device_type='cuda'):
        assert 0 <= fill <= 255
        self.fill, self.band_bytes, self.device_type = fill, max(int(band_bytes), 1), device_type
        self.regions = []          # every allocation made while active
        self.workspaces = []       # nbytes of every workspace.alloc call, in order
        self.outputs = []          # (shape, dtype) of every guarded empty / empty_like / zeros, in order

    # ---- which requests are guarded -------------------------------------------------------------------------------
    def _wants(self, device, dtype, kwargs):
        if device is None:
            return False
        device = torch.device(device)
        if device.type != self.device_type:
            return False
        if kwargs.get('memory_format', torch.contiguous_format) is not torch.contiguous_format:
            return False
        if kwargs.get('layout', torch.strided) is not torch.strided or kwargs.get('out') is not None or kwargs.get('names') is not None:
            return False
        return True

    def _tensor(self, shape, dtype, device, zero, requires_grad=False):
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        itemsize = _REAL_EMPTY(0, dtype=dtype).element_size()
        nbytes = _numel(shape) * itemsize
        r = _region('%s tensor of shape %s' % (str(dtype).replace('torch.', ''), tuple(shape)), nbytes, 0, self.band_bytes, self.fill, device)
        self.regions.append(r)
        self.outputs.append((tuple(shape), dtype))
        t = _interior(r, shape, dtype)
        if zero:
            t.zero_()
        if requires_grad:
            t.requires_grad_(True)
        return t

    # ---- the three replacements -----------------------------------------------------------------------------------
    def alloc(self, nbytes, device):
        nbytes = int(nbytes)
        r = _region('workspace of %d bytes' % nbytes, nbytes, SLACK, self.band_bytes, self.fill, device)
        self.regions.append(r)
        self.workspaces.append(nbytes)
        return _interior(r, (nbytes + SLACK,), torch.uint8)

    def empty(self, *args, **kwargs):
        if not self._wants(kwargs.get('device'), kwargs.get('dtype'), kwargs) or kwargs.get('pin_memory'):
            return _REAL_EMPTY(*args, **kwargs)
        return self._tensor(_shape_of(args, {k: v for k, v in kwargs.items() if k == 'size'}), kwargs.get('dtype'), kwargs['device'], False,
                            kwargs.get('requires_grad', False))

    def zeros(self, *args, **kwargs):
        if not self._wants(kwargs.get('device'), kwargs.get('dtype'), kwargs) or kwargs.get('pin_memory'):
            return _REAL_ZEROS(*args, **kwargs)
        return self._tensor(_shape_of(args, {k: v for k, v in kwargs.items() if k == 'size'}), kwargs.get('dtype'), kwargs['device'], True,
                            kwargs.get('requires_grad', False))

    def empty_like(self, t, **kwargs):
        device = kwargs.get('device', t.device)
        fmt = kwargs.get('memory_format', torch.preserve_format)
        dense = t.is_contiguous() or fmt is torch.contiguous_format      # preserve_format of a contiguous tensor is contiguous
        probe = dict(kwargs)
        probe['memory_format'] = torch.contiguous_format if dense and fmt in (torch.preserve_format, torch.contiguous_format) else fmt
        if not self._wants(device, None, probe) or t.layout is not torch.strided or kwargs.get('pin_memory'):
            return _REAL_EMPTY_LIKE(t, **kwargs)
        return self._tensor(tuple(t.shape), kwargs.get('dtype', t.dtype), device, False, kwargs.get('requires_grad', False))

    # ---- what the tests ask ---------------------------------------------------------------------------------------
    def check(self):
        """Synchronise, then assert that every band (and every workspace's slack) still holds `fill`."""
        if self.device_type == 'cuda':
            torch.cuda.synchronize()
        hits = [d for d in (r.damage() for r in self.regions) if d]
        assert not hits, 'guard bytes were written:\n  ' + '\n  '.join(hits)

    def saw_workspace(self, nbytes):
        return int(nbytes) in self.workspaces

    def saw_output(self, shape, dtype=None):
        return any(s == tuple(shape) and (dtype is None or d == dtype) for s, d in self.outputs)


@contextlib.contextmanager
def guarded(fill, band_bytes=MIN_BAND, device_type='cuda'):
    """Patch workspace.alloc, torch.empty, torch.empty_like and torch.zeros; restore them on exit, whatever happened."""
    from neural_ode_features_amd import workspace
    g = Guard(fill, band_bytes, device_type)
    saved = (workspace.alloc, torch.empty, torch.empty_like, torch.zeros)
    workspace.alloc, torch.empty, torch.empty_like, torch.zeros = g.alloc, g.empty, g.empty_like, g.zeros
    try:
        yield g
    finally:
        workspace.alloc, torch.empty, torch.empty_like, torch.zeros = saved


class Embedded:
    """An input inside a banded allocation, with the copy it must still equal after the call."""

    def __init__(self, tensor, region, saved):
        self.tensor, self.region, self.saved = tensor, region, saved

    def check(self):
        if self.tensor.is_cuda:
            torch.cuda.synchronize()
        d = self.region.damage()
        assert d is None, 'the bands around an input were written: ' + d
        now = self.tensor.detach().cpu().reshape(-1).view(torch.uint8)
        assert torch.equal(now, self.saved), 'an input was changed by the call: %s' % self.region.what


def embed_region(t, fill, band_bytes=MIN_BAND, device=None):
    """Copy `t` (contiguous) into the middle of a banded allocation on `device` (default: t's).  Returns an Embedded."""
    src = t.detach().contiguous()
    device = torch.device(device) if device is not None else src.device
    nbytes = src.numel() * src.element_size()
    r = _region('input %s of shape %s' % (str(src.dtype).replace('torch.', ''), tuple(src.shape)), nbytes, 0, band_bytes, fill, device)
    inner = _interior(r, src.shape, src.dtype)
    inner.copy_(src)
    saved = src.cpu().reshape(-1).view(torch.uint8).clone()
    return Embedded(inner, r, saved)


def embed(t, fill, band_bytes=MIN_BAND, device=None):
    """The interior tensor of `embed_region`: 256-byte aligned, equal to `t`, between bands of `fill`."""
    return embed_region(t, fill, band_bytes, device).tensor


# ---- the checks of one case -----------------------------------------------------------------------------------------

class Case:
    """One node on one shape.

    build()            -> list of CPU tensors (inputs, cotangents, parameters, labels), made from a seed
    run(tensors)       -> list of result tensors (outputs, every gradient, statistics); `tensors` are build()'s, on the
                          device (embedded in banded allocations for the guarded runs).  Must not keep references.
    calls              -> names of the library's entry points (`node_*_fwd`, ...) that the run must have called: a wrapper whose
                          `usable` check sends the call to ATen instead (alignment, hooks, capture) fails here
    bytes_fn           -> name of the library's `*_workspace_bytes` function: the run must have asked workspace.alloc for
                          exactly a figure this function returned to the wrapper
    workspaces(tensors)-> further byte counts of which each must have been asked of workspace.alloc, exactly
    outputs            -> [(shape, dtype)] (or a function that returns them) that must have been created through the guarded torch.empty / empty_like
    pools              -> the dict-like workspace pools to empty before a guarded run (restored afterwards)
    zero_scratch()     -> tensors whose contract is "all zero bits after the call" (looked up after the run)
    writes             -> indices of build()'s tensors that the node updates in place (optimiser steps): they are results,
                          not inputs; only the bands around them are checked
    """

    def __init__(self, name, build, run, workspaces=None, outputs=(), pools=(), zero_scratch=None, writes=(), calls=(), bytes_fn=None):
        self.name, self.build, self.run = name, build, run
        self.calls, self.bytes_fn = list(calls), bytes_fn
        self.workspaces = workspaces or (lambda tensors: [])
        self.outputs, self.pools, self.zero_scratch, self.writes = outputs, list(pools), zero_scratch, set(writes)

    def __repr__(self):
        return self.name


def _first_difference(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return 'shape/dtype %s %s against %s %s' % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    bad = ((a != b) | (a != a)).nonzero().reshape(-1)
    i = int(bad[0]) if bad.numel() else 0
    return '%d of %d elements differ, first at flat index %d: %r against %r' % (int(bad.numel()), a.numel(), i, a[i].item(), b[i].item())


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


@contextlib.contextmanager
def spied(names):
    """Record what the library's functions `names` return while active (set and restore on the loaded library object)."""
    log = {n: [] for n in names}
    if not names:
        yield log
        return
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    real = {n: getattr(lib, n) for n in names}

    def spy(name):
        def call(*args):
            r = real[name](*args)
            log[name].append(r)
            return r
        return call
    for n in names:
        setattr(lib, n, spy(n))
    try:
        yield log
    finally:
        for n in names:
            setattr(lib, n, real[n])


def plain_run(case, device):
    """Step 1: nothing patched, run twice, bit for bit the same.  Returns the results (on the CPU)."""
    tensors = case.build()
    first = [r.detach().cpu().clone() for r in case.run([t.to(device).clone() for t in tensors])]
    again = [r.detach().cpu().clone() for r in case.run([t.to(device).clone() for t in tensors])]
    _sync(device)
    assert len(first) == len(again)
    for k, (a, b) in enumerate(zip(first, again)):
        assert torch.equal(a, b), '%s is not bit-reproducible: result %d of two plain runs: %s' % (case.name, k, _first_difference(b, a))
    return first


def guarded_run(case, fill, plain, device, compare=True):
    """Step 2 for one fill.  `plain` is plain_run's list; compare=False leaves the cross-fill equality out (a node recorded
    as not bit-reproducible keeps its band and input checks)."""
    device = torch.device(device)
    tensors = case.build()
    saved_pools = [dict(p) for p in case.pools]
    for p in case.pools:
        p.clear()
    try:
        held = [embed_region(t, fill, device=device) for t in tensors]
        with spied(case.calls + ([case.bytes_fn] if case.bytes_fn else [])) as log, guarded(fill, device_type=device.type) as g:
            results = case.run([e.tensor for e in held])
            _sync(device)
        # the node ran: the library was called, its workspace was asked for with exactly the planned bytes, its outputs were made here
        for name in case.calls:
            assert log[name], '%s did not run its HIP node (fill 0x%02X): %s was never called' % (case.name, fill, name)
        if case.bytes_fn:
            planned = [v for v in log[case.bytes_fn] if v > 0]
            assert any(g.saw_workspace(v) for v in planned), (
                '%s did not run its HIP node (fill 0x%02X): %s returned %s, no workspace of exactly that size was allocated; seen %s'
                % (case.name, fill, case.bytes_fn, log[case.bytes_fn], g.workspaces))
        for nbytes in case.workspaces([e.tensor for e in held]):
            assert g.saw_workspace(nbytes), ('%s did not run its HIP node (fill 0x%02X): no workspace of exactly %d bytes was allocated; seen %s'
                                             % (case.name, fill, nbytes, g.workspaces))
        for shape, dtype in (case.outputs() if callable(case.outputs) else case.outputs):
            assert g.saw_output(shape, dtype), ('%s did not run its HIP node (fill 0x%02X): no %s output of shape %s was created; seen %s'
                                                % (case.name, fill, dtype, tuple(shape), g.outputs))
        # bands: workspaces with their slack, every output and gradient
        g.check()
        # inputs: unchanged, bands intact
        for k, e in enumerate(held):
            if k in case.writes:
                d = e.region.damage()
                assert d is None, 'the bands around an updated tensor were written: ' + d
            else:
                e.check()
        # results: the plain run's, bit for bit
        assert len(results) == len(plain)
        if compare:
            for k, (a, b) in enumerate(zip(results, plain)):
                assert torch.equal(a.detach().cpu(), b), (
                    '%s: result %d depends on bytes the node does not own (fill 0x%02X: an element never written, scratch read '
                    'before it is written, or an input read past its end): %s' % (case.name, k, fill, _first_difference(a, b)))
        if case.zero_scratch is not None:
            for z in case.zero_scratch():
                assert not bool(z.view(torch.uint8).any()), '%s left its zero-contract scratch non-zero (fill 0x%02X)' % (case.name, fill)
        return g
    finally:
        for p, s in zip(case.pools, saved_pools):
            p.clear()
            p.update(s)


def verify(case, device, compare=True):
    plain = plain_run(case, device)
    for fill in FILLS:
        guarded_run(case, fill, plain, device, compare)

"""A whole solve of `norm='batch'` dynamics inside the library (`node_bnsolve_fwd / node_bnsolve_adjoint`, csrc/bnsolve_api.hip).

`bnfunc.py` made ONE evaluation of `ODEfunc(C, norm='batch')` a HIP node; the solve around it stayed the generic solver's Python
loop (generic.py), which treats the node as a foreign `nn.Module`: parameters prepared again for every evaluation, an NCHW <-> NHWC
launch on either side of it, and in the adjoint a `torch.autograd.grad` followed by about fourteen small launches that copy the
results into the stage-derivative slots with the time sign.  Here the library drives the same step controller (`node_flat_*`)
itself: the state stays in the BatchNorm kernels' NHWC layout from the first stage to the last, the parameters are prepared once
per solve, and no Python or autograd runs between two evaluations.

Opt-in per function: `ODEfunc.batch_solve` is False by default (the library's behaviour without the switch is the generic
solver on the node); `resnet.build_model` sets it on the `norm='batch'` models it builds.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib, bnfunc, workspace

_HINT: Dict[tuple, int] = {}      # dopri5 steps per interval the last solve of the same problem took (enqueued before the first read-back)
_SCRATCH = workspace.Scratch()    # (device, stream, kind, shape, method, n_t) -> workspace; nothing is carried from a forward to its backward


def _stats(st):
    return {'nfe': st.nfe, 'accepted': st.accepted, 'rejected': st.rejected, 'status': st.status, 'last_dt': st.last_dt,
            't_final': st.t_final, 'first_dt': st.first_dt}


def _learn(key, st, intervals):
    tried = st.accepted + st.rejected
    _HINT[key] = max(1, -(-tried // intervals))
    if len(_HINT) > 256:
        _HINT.pop(next(iter(_HINT)))


def _params_struct(tensors):
    return _lib.NodeBnfuncParams(*[t.data_ptr() for t in tensors])


def _workspace(lib, dev, shape_args, method_id, adjoint, n_t):
    shape = _lib.NodeBnfuncShape(*shape_args)
    nbytes = lib.node_bnsolve_workspace_bytes(C.byref(shape), method_id, 1 if adjoint else 0, n_t)
    if nbytes == 0:
        _lib.unsupported()
    return shape, _SCRATCH.take(dev, nbytes, 'adj' if adjoint else 'fwd', shape_args, method_id, n_t), nbytes


class _BnOdeint(torch.autograd.Function):
    """Forward = `node_bnsolve_fwd`; backward = `node_bnsolve_adjoint`, the continuous adjoint -- for `odeint` too, as the generic
    solver does (upstream differentiates through the solver's own operations there: the same gradient up to O(tolerance)).
    `last_only`: the caller keeps y(t[-1]) alone and its gradient arrives as that one slice (`grad_last_only`), as in `_HipOdeint`."""

    @staticmethod
    def forward(ctx, func, eps, times, rtol, atol, method_id, max_steps, last_only, y0, *params):
        lib = _lib.load()
        y0 = y0.detach().contiguous()
        dev = y0.device
        n, c, h, w = y0.shape
        shape_args = (n, c, h, w, eps)
        ps = [p.detach().contiguous() for p in params]
        n_t = len(times)
        key = ('fwd', shape_args, method_id, rtol, atol, tuple(times))
        with torch.cuda.device(dev):
            shape, ws, nbytes = _workspace(lib, dev, shape_args, method_id, False, n_t)
            out = torch.empty((n_t,) + tuple(y0.shape), dtype=torch.float32, device=dev)
            opts = _lib.NodeBnsolveOpts(max_steps, _HINT.get(key, 1), 0)
            st = _lib.NodeStats()
            tarr = (C.c_float * n_t)(*times)
            rc = lib.node_bnsolve_fwd(C.byref(shape), C.byref(_params_struct(ps)), y0.data_ptr(), tarr, n_t, rtol, atol, method_id,
                                      C.byref(opts), out.data_ptr(), C.byref(st), workspace.aligned_ptr(ws), nbytes,
                                      torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc)
        if method_id == _lib.METHOD_DOPRI5:
            _learn(key, st, 1)
        func.nfe = getattr(func, 'nfe', 0) + st.nfe
        func.last_forward_stats = _stats(st)
        ctx.func, ctx.shape_args, ctx.times = func, shape_args, times
        ctx.rtol, ctx.atol, ctx.method_id, ctx.max_steps, ctx.last_only = rtol, atol, method_id, max_steps, bool(last_only)
        ctx.save_for_backward(out, *ps)
        return out[-1] if last_only else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        lib = _lib.load()
        out, *ps = ctx.saved_tensors
        dev = out.device
        n_t = len(ctx.times)
        grad_out = grad_out.contiguous()
        if grad_out.dtype != torch.float32:
            grad_out = grad_out.float()
        key = ('bwd', ctx.shape_args, ctx.method_id, ctx.rtol, ctx.atol, tuple(ctx.times))
        with torch.cuda.device(dev):
            shape, ws, nbytes = _workspace(lib, dev, ctx.shape_args, ctx.method_id, True, n_t)
            gy0 = torch.empty_like(out[0])
            grads = [torch.empty_like(p) for p in ps]
            opts = _lib.NodeBnsolveOpts(ctx.max_steps, _HINT.get(key, 1), 1 if ctx.last_only else 0)
            st = _lib.NodeStats()
            tarr = (C.c_float * n_t)(*ctx.times)
            rc = lib.node_bnsolve_adjoint(C.byref(shape), C.byref(_params_struct(ps)), out.data_ptr(), grad_out.data_ptr(), tarr, n_t,
                                          ctx.rtol, ctx.atol, ctx.method_id, C.byref(opts), gy0.data_ptr(),
                                          C.byref(_params_struct(grads)), C.byref(st), workspace.aligned_ptr(ws), nbytes,
                                          torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc)
        if ctx.method_id == _lib.METHOD_DOPRI5:
            _learn(key, st, n_t - 1)
        ctx.func.nfe = getattr(ctx.func, 'nfe', 0) + st.nfe
        ctx.func.last_backward_stats = _stats(st)
        need = ctx.needs_input_grad
        pg = [g if nd else None for g, nd in zip(grads, need[9:])]
        return (None, None, None, None, None, None, None, None, gy0 if need[8] else None, *pg)


def plan(func, y0, method_id, options, n_t=2):
    """(eps, the ten parameters, max_num_steps) when the library solves this problem itself, else None (-> the generic solver):
    `func` is the reference's `ODEfunc` with norm='batch' as `bnfunc._norms_and_convs` recognises it (no hooks, no tracked
    statistics) with both switches on (`fused_batch`, `batch_solve`); an fp32 NCHW state on a HIP device of a shape the
    workspace query takes for `n_t` time points, parameters fp32 on that device; `options` holds nothing but `max_num_steps`."""
    if not (getattr(func, 'fused_batch', False) and getattr(func, 'batch_solve', False)):
        return None
    if options and any(k != 'max_num_steps' for k in options):
        return None
    if not (torch.is_tensor(y0) and y0.is_cuda and y0.dtype == torch.float32 and y0.dim() == 4 and y0.shape[0] >= 1):
        return None
    if not all(hasattr(func, k) for k in ('norm1', 'norm2', 'norm3', 'conv1', 'conv2')):
        return None
    found = bnfunc._norms_and_convs(func)
    if found is None:
        return None
    eps, ps = found
    n, c, h, w = y0.shape
    if c != ps[0].shape[0] or not all(p.is_cuda and p.dtype == torch.float32 and p.device == y0.device for p in ps):
        return None
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():       # (the solve reads its controller back)
        return None
    shape = _lib.NodeBnfuncShape(n, c, h, w, eps)
    if _lib.load().node_bnsolve_workspace_bytes(C.byref(shape), method_id, 1, n_t) == 0:
        return None
    max_steps = int((options or {}).get('max_num_steps', 0) or 0)
    return eps, ps, max_steps


def odeint_batch(func, taken, y0, times, rtol, atol, method_id, last_only=False):
    eps, ps, max_steps = taken
    return _BnOdeint.apply(func, eps, list(times), float(rtol), float(atol), method_id, max_steps, last_only, y0, *ps)

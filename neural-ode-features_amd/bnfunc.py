"""`norm='batch'` dynamics as one autograd node (`node_bnfunc_fwd / node_bnfunc_bwd`, csrc/bnfunc_api.hip).

The reference's `--norm batch` (`train.py:202`, `model.py:268-281`) makes the three norms of `ODEfunc`
`nn.BatchNorm2d(dim, track_running_stats=False)`: batch statistics in training and evaluation alike.  BatchNorm couples the
samples of a batch, so the fused ODE block does not take it and such solves run the generic solver (generic.py), which calls
`func(t, y)` for every function evaluation -- about 14 times forward and 45 times in the adjoint of a CIFAR training step,
each adjoint evaluation followed by a `torch.autograd.grad` through it.  THAT evaluation is this node: BatchNorm passes with
two-stage statistics around the stem's gather-GEMM convolutions, the time channel of `ConcatConv2d` as an additive term, one
backward that returns the gradients of `t`, `x` and the ten parameters.  The step controller stays the generic solver's.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, workspace

_FREE = workspace.Carried()       # (device, shape) -> workspaces whose backward has run: free for the next forward of that shape
_SCRATCH = workspace.Scratch()    # (device, stream, shape) -> the workspace of forwards that keep nothing


def _struct(tensors):
    return _lib.NodeBnfuncParams(*[t.data_ptr() for t in tensors])


class _BatchOdeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, x, eps, keep, *params):
        lib = _lib.load()
        x = x.detach().contiguous()
        n, c, h, w = x.shape
        shape_args = (n, c, h, w, eps)
        shape = _lib.NodeBnfuncShape(*shape_args)
        dev = x.device
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            if torch.is_tensor(t):
                tdev = t.detach().to(device=dev, dtype=torch.float32).reshape(1)
            else:
                tdev = torch.full((1,), float(t), dtype=torch.float32, device=dev)     # a fill: no host-to-device copy
            nbytes = lib.node_bnfunc_workspace_bytes(C.byref(shape), 1 if keep else 0)
            if nbytes == 0:
                _lib.unsupported()
            if keep:
                # the workspace carries this forward's activations to its backward: one per forward in flight
                key = (dev.index,) + shape_args
                ws = _FREE.take(key, dev, nbytes)
            else:
                ws = _SCRATCH.take(dev, nbytes, *shape_args)
            out = torch.empty_like(x)
            _lib.check(lib.node_bnfunc_fwd(C.byref(shape), C.byref(_struct(ps)), tdev.data_ptr(), x.data_ptr(), out.data_ptr(),
                                           1 if keep else 0, workspace.aligned_ptr(ws), nbytes,
                                           torch.cuda.current_stream(dev).cuda_stream))
        ctx.ws = None
        if keep:
            ctx.shape_args, ctx.ws, ctx.nbytes, ctx.key = shape_args, ws, nbytes, key
            ctx.t_shape = tuple(t.shape) if torch.is_tensor(t) else None
            ctx.save_for_backward(tdev, *ps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if ctx.ws is None:
            raise RuntimeError('the fused batch-norm dynamics keep their activations in a workspace that the first backward releases: '
                               'a second backward through the same forward (retain_graph=True) is not supported')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ODEfunc: the fused backward does not run inside a stream capture')
        lib = _lib.load()
        tdev, *ps = ctx.saved_tensors
        shape = _lib.NodeBnfuncShape(*ctx.shape_args)
        dev = tdev.device
        grad_out = grad_out.contiguous()
        if grad_out.dtype != torch.float32:
            grad_out = grad_out.float()
        need = ctx.needs_input_grad
        want_t = need[0] and ctx.t_shape is not None
        want_x, want_p = need[1], any(need[4:])
        ws = ctx.ws
        with torch.cuda.device(dev):
            grads = [torch.empty_like(p) for p in ps] if want_p else None
            dx = torch.empty_like(grad_out) if want_x else None
            dt = torch.empty(1, dtype=torch.float32, device=dev) if want_t else None
            _lib.check(lib.node_bnfunc_bwd(C.byref(shape), C.byref(_struct(ps)), tdev.data_ptr(), grad_out.data_ptr(),
                                           C.byref(_struct(grads)) if want_p else None,
                                           dx.data_ptr() if want_x else None, dt.data_ptr() if want_t else None,
                                           workspace.aligned_ptr(ws), ctx.nbytes, torch.cuda.current_stream(dev).cuda_stream))
        _FREE.give(ctx.key, ws)       # free for the next forward of this shape (stream-ordered behind this backward)
        ctx.ws = None
        pg = [g if nd else None for g, nd in zip(grads, need[4:])] if want_p else [None] * len(ps)
        return (dt.reshape(ctx.t_shape) if want_t else None, dx, None, None, *pg)


def _norms_and_convs(func):
    """(eps, the ten tensors in node_bnfunc_params order), or None if `func` is not the reference's ODEfunc with norm='batch':
    three `nn.BatchNorm2d(C, track_running_stats=False)` with affine parameters, two `ConcatConv2d` over a
    `nn.Conv2d(C + 1, C, 3, 1, 1)` with bias; no hooks on any of them."""
    from .modules import ConcatConv2d
    norms = (func.norm1, func.norm2, func.norm3)
    convs = (func.conv1, func.conv2)
    c = getattr(norms[0], 'num_features', None)
    for m in norms:
        if not isinstance(m, nn.BatchNorm2d) or not m.affine or m.track_running_stats or m.running_mean is not None:
            return None
        if m.num_features != c or m.eps != norms[0].eps or m._forward_hooks or m._forward_pre_hooks:
            return None
    for m in convs:
        if not isinstance(m, ConcatConv2d) or m._forward_hooks or m._forward_pre_hooks:
            return None
        conv = m._layer
        if not isinstance(conv, nn.Conv2d) or conv.bias is None or conv._forward_hooks or conv._forward_pre_hooks:
            return None
        if (conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode) != \
                ((3, 3), (1, 1), (1, 1), (1, 1), 1, 'zeros') or conv.in_channels != c + 1 or conv.out_channels != c:
            return None
    if func._forward_hooks or func._forward_pre_hooks:
        return None
    ps = [func.norm1.weight, func.norm1.bias, func.conv1._layer.weight, func.conv1._layer.bias,
          func.norm2.weight, func.norm2.bias, func.conv2._layer.weight, func.conv2._layer.bias,
          func.norm3.weight, func.norm3.bias]
    return float(norms[0].eps), ps


def _time_ok(t, x):
    """A Python number, or a one-element real tensor: on x's device, or on the CPU without a gradient wanted (read as a number)."""
    if isinstance(t, (int, float)):
        return True
    if not (torch.is_tensor(t) and t.numel() == 1 and t.is_floating_point()):
        return False
    return t.device == x.device or (t.device.type == 'cpu' and not t.requires_grad)


def plan(func, t, x):
    """What `evaluate` needs, or None if the library does not take this call (node_bnfunc_fwd): an fp32 NCHW batch on a HIP
    device, channels a multiple of 64 in [64, 4096], h, w >= 3, tensors under 2^31 elements, parameters fp32 on the input's
    device.  Anything else -- the 16- and 96-filter nets of the tests, CPU or fp64 tensors -- runs the module operations."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1):
        return None
    if x.is_contiguous() and x.data_ptr() % 16:       # (a view at an odd offset: the kernels load 16 bytes at a time)
        return None
    found = _norms_and_convs(func)
    if found is None or not _time_ok(t, x):
        return None
    eps, ps = found
    n, c, h, w = x.shape
    if not (c == ps[0].shape[0] and 64 <= c <= 4096 and c % 64 == 0 and h >= 3 and w >= 3 and (n * h * w + 1) * c < 2 ** 31
            and all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in ps)):
        return None
    keep = torch.is_grad_enabled() and (x.requires_grad or (torch.is_tensor(t) and t.requires_grad) or any(p.requires_grad for p in ps))
    if keep and torch.cuda.is_current_stream_capturing():
        return None
    return eps, ps, keep


def evaluate(t, x, eps, ps, keep):
    if torch.is_tensor(t) and t.device != x.device:
        t = float(t)
    if not keep:
        ps = [p.detach() for p in ps]
    return _BatchOdeFn.apply(t, x, eps, keep, *ps)

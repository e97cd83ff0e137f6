"""The 4x4 stride-2 convolution that turns the image into the ODE block's state -- the whole of the reference's one-shot stem
(`model.py:119-126`) and the `conv1` of its `ode` / `ode2` stems (`model.py:185, 203`) -- forward and backward through the
HIP library (`node_imgconv_fwd / node_imgconv_bwd`, csrc/kernels_imgconv.hip).  `ImageConv2d` IS an `nn.Conv2d` (same
parameters, same state_dict keys); CPU tensors, non-fp32 inputs and geometries the kernels do not take (the 16-filter nets of the
fixtures, odd image sides) run `nn.Conv2d.forward` -- on a HIP device with the library missing, the fused path raises.  The
backward also returns the input gradient when the input asks for one: the package's HIP path from the loss to the pixels.

Two limits.  The backward is first order only (`once_differentiable`: a `create_graph=True` backward through it raises).  And the
fused backward stays out of stream captures: a forward that is being captured with gradients wanted
(`torch.cuda.make_graphed_callables`, `graphs.capture_static_parts`) takes `nn.Conv2d.forward`, as it did before this class
existed, and a backward that finds itself in a capture raises.  Captured inference (`graphs.capture_inference`, no gradients)
runs the fused forward.  The backward's scratch is one buffer per (device, stream, shape), allocated by the forward that will need
it, so backwards of one shape on two streams do not share it.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, workspace

_WS = workspace.Scratch()


def _workspace(lib, shape, shape_args, dev):
    """The backward's scratch (aligned pointer, bytes), one per (device, stream, shape): it carries nothing between calls, and calls
    on one stream are ordered.  Autograd runs a node's backward on its forward's stream, so the buffer the forward made is the one
    the backward finds."""
    nbytes = lib.node_imgconv_workspace_bytes(C.byref(shape))
    if nbytes == 0:
        _lib.unsupported()
    return workspace.aligned_ptr(_WS.take(dev, nbytes, *shape_args)), nbytes


class _ImgConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, prepare):
        lib = _lib.load()
        x = x.detach().contiguous()
        w = weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        n, cin, h, wd = x.shape
        filters = w.shape[0]
        shape = _lib.NodeImgConvShape(n, cin, h, wd, filters)
        dev = x.device
        with torch.cuda.device(dev):
            y = torch.empty(n, filters, h // 2, wd // 2, dtype=torch.float32, device=dev)
            _lib.check(lib.node_imgconv_fwd(C.byref(shape), x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                            y.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            if prepare:                            # the backward's scratch exists before the backward runs; never made in a capture
                _workspace(lib, shape, (n, cin, h, wd, filters), dev)
        ctx.shape_args = (n, cin, h, wd, filters)
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ImageConv2d: the fused backward does not run inside a stream capture; capture the forward with '
                               'it (it then takes nn.Conv2d.forward) or run this backward outside the capture')
        lib = _lib.load()
        x, w = ctx.saved_tensors
        shape = _lib.NodeImgConvShape(*ctx.shape_args)
        dev = x.device
        grad_y = grad_y.contiguous()
        if grad_y.dtype != torch.float32:
            grad_y = grad_y.float()
        want_x = ctx.needs_input_grad[0]
        with torch.cuda.device(dev):
            dw = torch.empty_like(w)
            db = torch.empty(w.shape[0], dtype=torch.float32, device=dev) if ctx.has_bias else None
            dx = torch.empty_like(x) if want_x else None
            ws, nbytes = _workspace(lib, shape, ctx.shape_args, dev)
            _lib.check(lib.node_imgconv_bwd(C.byref(shape), x.data_ptr(), w.data_ptr(), grad_y.data_ptr(), dw.data_ptr(),
                                            db.data_ptr() if db is not None else None, dx.data_ptr() if dx is not None else None,
                                            ws, nbytes, torch.cuda.current_stream(dev).cuda_stream))
        return dx, dw, db, None


def _wants_grad(conv, x) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in conv.parameters(recurse=False)))


def fusable(conv, x) -> bool:
    """What the library's kernels take (node_imgconv_fwd): a 4x4 / stride 2 / padding 1 convolution of an fp32 NCHW batch on a HIP
    device with at most 4 input channels, even sides >= 4 and a multiple of 64 filters, parameters fp32 on the same device."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if (conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode) != \
            ((4, 4), (2, 2), (1, 1), (1, 1), 1, 'zeros'):
        return False
    n, cin, h, w = x.shape
    if not (n >= 1 and cin == conv.in_channels and 1 <= cin <= 4 and h >= 4 and w >= 4 and h % 2 == 0 and w % 2 == 0
            and conv.out_channels % 64 == 0):
        return False
    ps = [conv.weight] + ([conv.bias] if conv.bias is not None else [])
    return all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in ps)


class ImageConv2d(nn.Conv2d):
    """`nn.Conv2d(in_ch, filters, 4, 2, 1)` whose forward, weight / bias gradient and input gradient are the library's kernels
    on a HIP device (one autograd node; x and the weight are all it saves, so a second backward with retain_graph works).  A
    forward captured into a graph with gradients wanted takes the parent path: the fused backward is kept out of captures."""

    def __init__(self, in_channels, out_channels, kernel_size=4, stride=2, padding=1, **kw):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, **kw)

    def forward(self, x):
        if not fusable(self, x) or (_wants_grad(self, x) and torch.cuda.is_current_stream_capturing()):
            return super().forward(x)
        return _ImgConvFn.apply(x, self.weight, self.bias, _wants_grad(self, x))

"""The hand-off between the two solves of the `ode2` stem -- `conv2(norm(x))` of `ODEDownsample2`,
`/root/reference/model.py:199-223`: GroupNorm -> ReLU -> `nn.Conv2d(C, C, 4, 2, 1)` -- forward and backward through the HIP
library (`node_downconv_fwd / node_downconv_bwd`, csrc/downconv_api.hip on the kernels of csrc/kernels_stem.hip): ONE
autograd node, NHWC inside, no MIOpen call, no layout transposes, no PyTorch reductions.  `gn_relu_conv(x, gn, conv)` takes
the plain modules as parameter containers; CPU tensors, non-fp32 inputs, shapes the kernels refuse, another norm or
convolution and a stream that is being captured run those modules -- on a HIP device with the library missing, the fused
path raises.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib, workspace

_WS = workspace.Carried(keep=1)      # (device, shape) -> the workspace whose backward has run
_FWD = workspace.Scratch()           # forwards that no backward follows (inference): nothing is carried


def _struct(tensors):
    return _lib.NodeDownConvParams(*[t.data_ptr() for t in tensors])


class _DownConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, keep, gn_w, gn_b, conv_w, conv_b):
        lib = _lib.load()
        x = x.detach().contiguous()
        ps = [p.detach().contiguous() for p in (gn_w, gn_b, conv_w, conv_b)]
        n, cin, h, w = x.shape
        cout = conv_w.shape[0]
        shape = _lib.NodeDownConvShape(n, cin, cout, h, w, eps)
        dev = x.device
        with torch.cuda.device(dev):
            nbytes = lib.node_downconv_workspace_bytes(C.byref(shape), int(keep))
            if nbytes == 0:
                _lib.unsupported()
            key = (dev.index, n, cin, cout, h, w)
            # with a backward to come the workspace carries the activations to it: one per (device, shape) in flight
            ws = _WS.take(key, dev, nbytes) if keep else _FWD.take(dev, nbytes, *key[1:])
            y = torch.empty(n, cout, (h - 2) // 2 + 1, (w - 2) // 2 + 1, dtype=torch.float32, device=dev)
            _lib.check(lib.node_downconv_fwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), y.data_ptr(), int(keep),
                                             workspace.aligned_ptr(ws), nbytes, torch.cuda.current_stream(dev).cuda_stream))
        ctx.shape_args = (n, cin, cout, h, w, eps)
        ctx.ws, ctx.nbytes, ctx.key = (ws if keep else None), nbytes, key
        ctx.save_for_backward(*ps)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        lib = _lib.load()
        ps = ctx.saved_tensors
        if ctx.ws is None:
            raise RuntimeError('the fused hand-off keeps its activations in a workspace that the first backward releases: '
                               'a second backward through the same forward (retain_graph=True) is not supported')
        shape = _lib.NodeDownConvShape(*ctx.shape_args)
        n, cin, cout, h, w, _ = ctx.shape_args
        dev = grad_y.device
        grad_y = grad_y.contiguous()
        if grad_y.dtype != torch.float32:
            grad_y = grad_y.float()
        want_params = any(ctx.needs_input_grad[3:])      # all four or none (frozen parameters: the data-gradient chain alone)
        grads = [torch.empty_like(p) for p in ps] if want_params else None
        ws = ctx.ws
        with torch.cuda.device(dev):
            d_x = torch.empty(n, cin, h, w, dtype=torch.float32, device=dev)
            _lib.check(lib.node_downconv_bwd(C.byref(shape), C.byref(_struct(ps)), grad_y.data_ptr(),
                                             C.byref(_struct(grads)) if grads is not None else None, d_x.data_ptr(),
                                             workspace.aligned_ptr(ws), ctx.nbytes, torch.cuda.current_stream(dev).cuda_stream))
        _WS.give(ctx.key, ws)        # free for the next forward of this shape (stream-ordered behind this backward)
        ctx.ws = None
        if grads is None:
            grads = [None] * 4
        return (d_x if ctx.needs_input_grad[0] else None, None, None, *grads)


def fusable(x, gn, conv) -> bool:
    """What the library's kernels take (node_downconv_fwd): an fp32 NCHW batch on a HIP device, an affine
    GroupNorm(min(32, C), C), a 4x4 / stride 2 / padding 1 `zeros` convolution with bias, channel counts that are powers of
    two >= 64, sides >= 4 whose image fits the GroupNorm passes' LDS block -- and a stream that is not being captured."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1):
        return False
    if not (isinstance(gn, nn.GroupNorm) and gn.affine and gn.num_channels == x.shape[1]
            and gn.num_groups == min(32, gn.num_channels)):
        return False
    if not isinstance(conv, nn.Conv2d) or conv.bias is None or conv.in_channels != x.shape[1]:
        return False
    if (conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode) != \
            ((4, 4), (2, 2), (1, 1), (1, 1), 1, 'zeros'):
        return False
    ps = (gn.weight, gn.bias, conv.weight, conv.bias)
    if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in ps):
        return False
    if torch.cuda.is_current_stream_capturing():
        return False
    n, cin, h, w = x.shape
    shape = _lib.NodeDownConvShape(n, cin, conv.out_channels, h, w, gn.eps)
    return _lib.load().node_downconv_workspace_bytes(C.byref(shape), 1) != 0      # (0: refused, with a message)


def gn_relu_conv(x, gn, conv):
    """`conv(relu(gn(x)))`: one autograd node on the library's kernels where `fusable`, the modules otherwise."""
    if not fusable(x, gn, conv):
        from .head import gn_relu
        return conv(gn_relu(x, gn))
    ps = (gn.weight, gn.bias, conv.weight, conv.bias)
    keep = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))      # a backward may follow
    return _DownConvFn.apply(x, float(gn.eps), keep, *ps)

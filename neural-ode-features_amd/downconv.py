"""The hand-off between the two solves of the `ode2` stem -- `conv2(norm(x))` of `ODEDownsample2`,
`/root/reference/model.py:199-223`: GroupNorm -> ReLU -> `nn.Conv2d(C, C, 4, 2, 1)` -- forward and backward through the HIP
library (`node_downconv_fwd / node_downconv_bwd`, csrc/downconv_api.hip on the kernels of csrc/kernels_stem.hip): ONE
autograd node, NHWC inside, no MIOpen call, no layout transposes, no PyTorch reductions.  `gn_relu_conv(x, gn, conv)` takes
the plain modules as parameter containers; CPU tensors, non-fp32 inputs, shapes the kernels refuse, another norm or
convolution and a stream that is being captured run those modules -- on a HIP device with the library missing, the fused
path raises.

`bn_relu_conv(x, bn, conv, slices=1)` is the same hand-off of a `norm='batch'` net (`nn.BatchNorm2d(C,
track_running_stats=False)`, model.py:274): `node_bndownconv_fwd / node_bndownconv_bwd`, csrc/bndownconv_api.hip.  With
`slices` = T it takes a whole trajectory [T N, C, H, W] in ONE call, statistics per slice (the no-grad forward only).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

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


_BN_FREE = workspace.Carried()       # (device, shape) -> workspaces whose backward has run: free for the next forward of that shape
_BN_SCRATCH = workspace.Scratch()    # (device, stream, shape) -> the workspace of forwards that keep nothing


class _BnDownConvFn(torch.autograd.Function):
    """The `norm='batch'` hand-off: node_bndownconv_fwd / node_bndownconv_bwd (csrc/bndownconv_api.hip), with `stem._BnStemFn`'s
    workspace discipline.  `slices` > 1 (a trajectory's T slices as one batch of T N samples, statistics per slice) is the no-grad
    forward only: the library refuses it with a backward to come."""

    @staticmethod
    def forward(ctx, x, eps, keep, slices, bn_w, bn_b, conv_w, conv_b):
        lib = _lib.load()
        x = x.detach().contiguous()
        ps = [p.detach().contiguous() for p in (bn_w, bn_b, conv_w, conv_b)]
        n, cin, h, w = x.shape
        cout = conv_w.shape[0]
        shape_args = (n, cin, cout, h, w, slices, eps)
        shape = _lib.NodeBnDownConvShape(*shape_args)
        dev = x.device
        with torch.cuda.device(dev):
            nbytes = lib.node_bndownconv_workspace_bytes(C.byref(shape), 1 if keep else 0)
            if nbytes == 0:
                _lib.unsupported()
            if keep:
                key = (dev.index,) + shape_args
                ws = _BN_FREE.take(key, dev, nbytes)
            else:
                ws = _BN_SCRATCH.take(dev, nbytes, *shape_args)
            y = torch.empty(n, cout, (h - 2) // 2 + 1, (w - 2) // 2 + 1, dtype=torch.float32, device=dev)
            _lib.check(lib.node_bndownconv_fwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), y.data_ptr(), 1 if keep else 0,
                                               workspace.aligned_ptr(ws), nbytes, torch.cuda.current_stream(dev).cuda_stream))
        ctx.ws = None
        if keep:
            ctx.shape_args, ctx.ws, ctx.nbytes, ctx.key = shape_args, ws, nbytes, key
            ctx.save_for_backward(*ps)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        if ctx.ws is None:
            raise RuntimeError('the fused hand-off keeps its activations in a workspace that the first backward releases: '
                               'a second backward through the same forward (retain_graph=True) is not supported')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the fused hand-off\'s backward does not run inside a stream capture')
        lib = _lib.load()
        ps = ctx.saved_tensors
        shape = _lib.NodeBnDownConvShape(*ctx.shape_args)
        n, cin, cout, h, w, _, _ = ctx.shape_args
        dev = grad_y.device
        grad_y = grad_y.contiguous()
        if grad_y.dtype != torch.float32:
            grad_y = grad_y.float()
        if grad_y.data_ptr() % 16:
            grad_y = grad_y.clone()
        want_params = any(ctx.needs_input_grad[4:])      # all four or none (frozen parameters: the data-gradient chain alone)
        ws = ctx.ws
        with torch.cuda.device(dev):
            grads = [torch.empty_like(p) for p in ps] if want_params else None
            d_x = torch.empty(n, cin, h, w, dtype=torch.float32, device=dev)
            _lib.check(lib.node_bndownconv_bwd(C.byref(shape), C.byref(_struct(ps)), grad_y.data_ptr(),
                                               C.byref(_struct(grads)) if grads is not None else None, d_x.data_ptr(),
                                               workspace.aligned_ptr(ws), ctx.nbytes, torch.cuda.current_stream(dev).cuda_stream))
        _BN_FREE.give(ctx.key, ws)       # free for the next forward of this shape (stream-ordered behind this backward)
        ctx.ws = None
        if grads is None:
            grads = [None] * 4
        return (d_x if ctx.needs_input_grad[0] else None, None, None, None, *grads)


def _hooked(*mods):
    """a forward or backward hook on the norm or the convolution: the node would not call it"""
    return any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, '_backward_pre_hooks', None) for m in mods)


def bn_fusable(x, bn, conv, slices=1) -> bool:
    """What node_bndownconv_fwd takes: an fp32 NCHW batch on a HIP device (of `slices` equal slices), an affine
    `nn.BatchNorm2d(C, track_running_stats=False)` without running buffers, a 4x4 / stride 2 / padding 1 `zeros` convolution with
    bias, channel counts that are multiples of 64 in [64, 4096] (192 included), sides >= 4, 16-byte aligned fp32 tensors under 2^31
    elements on one device, no hooks on the two modules, no stream capture; `slices` > 1 only where no backward can follow."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1):
        return False
    if not (isinstance(bn, nn.BatchNorm2d) and bn.affine and not bn.track_running_stats and bn.running_mean is None
            and bn.num_features == x.shape[1]):
        return False
    if not isinstance(conv, nn.Conv2d) or conv.bias is None or conv.in_channels != x.shape[1]:
        return False
    if (conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.padding_mode) != \
            ((4, 4), (2, 2), (1, 1), (1, 1), 1, 'zeros'):
        return False
    if _hooked(bn, conv):
        return False
    ps = (bn.weight, bn.bias, conv.weight, conv.bias)
    if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device and p.data_ptr() % 16 == 0 for p in ps):
        return False
    n, cin, h, w = x.shape
    cout = conv.out_channels
    if not (cin % 64 == 0 and 64 <= cin <= 4096 and cout % 64 == 0 and 64 <= cout <= 4096 and min(h, w) >= 4
            and slices >= 1 and n % slices == 0 and n * h * w * max(cin, cout) + 4096 < 2 ** 31):
        return False
    if slices > 1 and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps)):
        return False
    return x.data_ptr() % 16 == 0 and not torch.cuda.is_current_stream_capturing()


def bn_relu_conv(x, bn, conv, slices=1):
    """`conv(relu(bn(x)))` for a `norm='batch'` hand-off: one autograd node on the library's kernels where `bn_fusable`, the
    modules otherwise.  `slices` = T > 1: `x` is a trajectory's T slices flattened to [T N, C, H, W]; every slice is normalised
    with its own statistics (the modules: T calls of `bn`)."""
    if not bn_fusable(x, bn, conv, slices):
        if slices > 1:
            xs = x.reshape(slices, x.shape[0] // slices, *x.shape[1:])
            return torch.cat([conv(F.relu(bn(xi))) for xi in xs])
        return conv(F.relu(bn(x)))
    ps = (bn.weight, bn.bias, conv.weight, conv.bias)
    keep = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))      # a backward may follow
    if not keep:
        ps = [p.detach() for p in ps]
    return _BnDownConvFn.apply(x, float(bn.eps), keep, int(slices), *ps)


def gn_relu_conv(x, gn, conv):
    """`conv(relu(gn(x)))`: one autograd node on the library's kernels where `fusable`, the modules otherwise."""
    if not fusable(x, gn, conv):
        from .head import gn_relu
        return conv(gn_relu(x, gn))
    ps = (gn.weight, gn.bias, conv.weight, conv.bias)
    keep = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))      # a backward may follow
    return _DownConvFn.apply(x, float(gn.eps), keep, *ps)

"""The `minimal` stem in front of the ODE block -- `MinimalConvDownsample`, the reference's `model.py:129-145`:
Conv2d(in_ch, 24, 3, 1) | GroupNorm(24, 24) + ReLU | Conv2d(24, 24, 4, 2, 1) | GroupNorm(24, 24) + ReLU |
Conv2d(24, filters, 4, 2, 1) -- forward and backward through the HIP library (`node_ministem_fwd / node_ministem_bwd`,
csrc/ministem_api.hip on the kernels of csrc/kernels_ministem.hip): ONE autograd node for the whole stem, NHWC inside, no
MIOpen call, no layout transposes, no PyTorch reductions.  `MinimalStem` IS the reference's `nn.Sequential` of seven children
(same state_dict keys: `0.weight`, `1.weight`, `3.weight`, ...), so checkpoints load unchanged; CPU tensors, non-fp32 inputs,
a stream that is being captured, shapes the kernels refuse and -- with `input_grad` off -- an input that requires a gradient
run the module sequence; on a HIP device with the library missing, the fused path raises.

A `norm='batch'` stem (both norms `nn.BatchNorm2d(24, track_running_stats=False)`, model.py:274) can be one node too:
`_BnMiniStemFn` (`node_bnministem_fwd / node_bnministem_bwd`, csrc/bnministem_api.hip), the same convolutions around the
BatchNorm passes of csrc/kernels_bnministem.hip.  It runs with `MinimalStem.fused_batch = True`; the switch ships False, which
runs the module sequence: the node's forward + backward measured slower than the modules at the CIFAR training shape
(profiles/bnministem_time.txt).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, workspace

MID = 24                             # the stem's middle channel count (model.py:133)
_WS = workspace.Carried(keep=1)      # (device, shape) -> the workspace whose backward has run
_FWD = workspace.Scratch()           # forwards that no backward follows (inference): nothing is carried


def _params_of(seq):
    """The ten tensors of the stem in node_ministem_params (= state_dict) order, or None if `seq` is not the reference's layout."""
    try:
        c0, n1, r1, c1, n2, r2, c2 = list(seq.children())
    except ValueError:
        return None
    if not (isinstance(r1, nn.ReLU) and isinstance(r2, nn.ReLU)):
        return None
    for conv, geom in ((c0, ((3, 3), (1, 1), (0, 0))), (c1, ((4, 4), (2, 2), (1, 1))), (c2, ((4, 4), (2, 2), (1, 1)))):
        if not isinstance(conv, nn.Conv2d) or conv.bias is None:
            return None
        if (conv.kernel_size, conv.stride, conv.padding) != geom or (conv.dilation, conv.groups, conv.padding_mode) != ((1, 1), 1, 'zeros'):
            return None
    for gn in (n1, n2):      # groups of one channel: GroupNorm(min(32, 24), 24)
        if not (isinstance(gn, nn.GroupNorm) and gn.affine and gn.num_channels == MID and gn.num_groups == MID and gn.eps == n1.eps):
            return None
    if (c0.out_channels, c1.in_channels, c1.out_channels, c2.in_channels) != (MID, MID, MID, MID):
        return None
    return [c0.weight, c0.bias, n1.weight, n1.bias, c1.weight, c1.bias, n2.weight, n2.bias, c2.weight, c2.bias]


def _struct(tensors):
    return _lib.NodeMiniStemParams(*[t.data_ptr() for t in tensors])


class _MiniStemFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, keep, *params):
        lib = _lib.load()
        x = x.detach().contiguous()
        ps = [p.detach().contiguous() for p in params]
        n, cin, h, w = x.shape
        filters = ps[-1].shape[0]
        shape = _lib.NodeMiniStemShape(n, cin, h, w, filters, eps)
        dev = x.device
        with torch.cuda.device(dev):
            nbytes = lib.node_ministem_workspace_bytes(C.byref(shape), int(keep))
            if nbytes == 0:
                _lib.unsupported()
            key = (dev.index, n, cin, h, w, filters)
            # with a backward to come the workspace carries the activations to it: one per (device, shape) in flight
            ws = _WS.take(key, dev, nbytes) if keep else _FWD.take(dev, nbytes, *key[1:])
            h2, w2 = ((h - 2 - 2) // 2 + 1 - 2) // 2 + 1, ((w - 2 - 2) // 2 + 1 - 2) // 2 + 1
            out = torch.empty(n, filters, h2, w2, dtype=torch.float32, device=dev)
            _lib.check(lib.node_ministem_fwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), out.data_ptr(), int(keep),
                                             workspace.aligned_ptr(ws), nbytes, torch.cuda.current_stream(dev).cuda_stream))
        ctx.shape_args = (n, cin, h, w, filters, eps)
        ctx.ws, ctx.nbytes, ctx.key = (ws if keep else None), nbytes, key
        ctx.save_for_backward(x, *ps)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        x, *ps = ctx.saved_tensors
        if ctx.ws is None:
            raise RuntimeError('the fused stem keeps its activations in a workspace that the first backward releases: '
                               'a second backward through the same forward (retain_graph=True) is not supported')
        shape = _lib.NodeMiniStemShape(*ctx.shape_args)
        dev = x.device
        grad_out = grad_out.contiguous()
        if grad_out.dtype != torch.float32:
            grad_out = grad_out.float()
        # parameter gradients: all ten or none (an attack freezes the parameters: the data-gradient chain alone)
        want_params = any(ctx.needs_input_grad[3:])
        want_dx = ctx.needs_input_grad[0]     # (only with MinimalStem.input_grad: `fusable` sends any other such input elsewhere)
        grads = [torch.empty_like(p) for p in ps] if want_params or not want_dx else None
        d_x = torch.empty_like(x) if want_dx else None
        ws = ctx.ws
        with torch.cuda.device(dev):
            _lib.check(lib.node_ministem_bwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), grad_out.data_ptr(),
                                             C.byref(_struct(grads)) if grads is not None else None,
                                             d_x.data_ptr() if d_x is not None else None, workspace.aligned_ptr(ws), ctx.nbytes,
                                             torch.cuda.current_stream(dev).cuda_stream))
        _WS.give(ctx.key, ws)        # free for the next forward of this shape (stream-ordered behind this backward)
        ctx.ws = None
        if grads is None:
            grads = [None] * len(ps)
        return (d_x, None, None, *grads)


def fusable(seq, x, input_grad=False) -> bool:
    """What the library's kernels take (node_ministem_fwd): fp32 on a HIP device, in_ch <= 3, filters a power of two in
    [64, 4096], images of 10 x 10 pixels and more; an input that requires a gradient only with `input_grad`; a capturing stream
    and anything else -- filters = 192 -- run the module sequence (`norm='batch'` children: `bn_fusable`)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1):
        return False
    if x.requires_grad and torch.is_grad_enabled() and not input_grad:
        return False
    ps = _params_of(seq)
    if ps is None or ps[0].shape[1] != x.shape[1]:
        return False
    if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in ps):
        return False
    if torch.cuda.is_current_stream_capturing():
        return False
    n, cin, h, w = x.shape
    shape = _lib.NodeMiniStemShape(n, cin, h, w, ps[-1].shape[0], seq[1].eps)
    return _lib.load().node_ministem_workspace_bytes(C.byref(shape), 1) != 0      # (0: refused, with a message)


def _bn_params_of(seq):
    """The same ten tensors for a `norm='batch'` stem, or None: the reference's layout with two
    `nn.BatchNorm2d(24, track_running_stats=False)` (model.py:274) -- affine, no running buffers (they would have to be updated in
    training and USED in evaluation: the node does neither), one eps -- and the convolution geometry `_params_of` asks for."""
    try:
        c0, n1, r1, c1, n2, r2, c2 = list(seq.children())
    except ValueError:
        return None
    if not (isinstance(r1, nn.ReLU) and isinstance(r2, nn.ReLU)):
        return None
    for conv, geom in ((c0, ((3, 3), (1, 1), (0, 0))), (c1, ((4, 4), (2, 2), (1, 1))), (c2, ((4, 4), (2, 2), (1, 1)))):
        if not isinstance(conv, nn.Conv2d) or conv.bias is None:
            return None
        if (conv.kernel_size, conv.stride, conv.padding) != geom or (conv.dilation, conv.groups, conv.padding_mode) != ((1, 1), 1, 'zeros'):
            return None
    for bn in (n1, n2):
        if not isinstance(bn, nn.BatchNorm2d) or not bn.affine or bn.track_running_stats or bn.running_mean is not None \
                or bn.eps != n1.eps or bn.num_features != MID:
            return None
    if (c0.out_channels, c1.in_channels, c1.out_channels, c2.in_channels) != (MID, MID, MID, MID):
        return None
    return [c0.weight, c0.bias, n1.weight, n1.bias, c1.weight, c1.bias, n2.weight, n2.bias, c2.weight, c2.bias]


def _out_size(h):
    return ((h - 2 - 2) // 2 + 1 - 2) // 2 + 1


_BN_FREE = workspace.Carried()       # (device, shape) -> workspaces whose backward has run: free for the next forward of that shape
_BN_SCRATCH = workspace.Scratch()    # (device, stream, shape) -> the workspace of forwards that keep nothing


class _BnMiniStemFn(torch.autograd.Function):
    """The `norm='batch'` minimal stem: node_bnministem_fwd / node_bnministem_bwd (csrc/bnministem_api.hip), with
    `convstem._BnConvStemFn`'s workspace discipline: a forward that wants gradients keeps its activations in a workspace of its own
    until its backward has run, a no-grad forward uses the stream's scratch and touches none of them."""

    @staticmethod
    def forward(ctx, x, eps, keep, *params):
        lib = _lib.load()
        x = x.detach().contiguous()
        n, cin, h, w = x.shape
        filters = params[-1].shape[0]
        shape_args = (n, cin, h, w, filters, eps)
        shape = _lib.NodeMiniStemShape(*shape_args)
        dev = x.device
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            nbytes = lib.node_bnministem_workspace_bytes(C.byref(shape), 1 if keep else 0)
            if nbytes == 0:
                _lib.unsupported()
            if keep:
                key = (dev.index,) + shape_args
                ws = _BN_FREE.take(key, dev, nbytes)
            else:
                ws = _BN_SCRATCH.take(dev, nbytes, *shape_args)
            out = torch.empty(n, filters, _out_size(h), _out_size(w), dtype=torch.float32, device=dev)
            _lib.check(lib.node_bnministem_fwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), out.data_ptr(), 1 if keep else 0,
                                               workspace.aligned_ptr(ws), nbytes, torch.cuda.current_stream(dev).cuda_stream))
        ctx.ws = None
        if keep:
            ctx.shape_args, ctx.ws, ctx.nbytes, ctx.key = shape_args, ws, nbytes, key
            ctx.save_for_backward(x, *ps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if ctx.ws is None:
            raise RuntimeError('the fused stem keeps its activations in a workspace that the first backward releases: '
                               'a second backward through the same forward (retain_graph=True) is not supported')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('MinimalStem: the fused backward does not run inside a stream capture')
        lib = _lib.load()
        x, *ps = ctx.saved_tensors
        shape = _lib.NodeMiniStemShape(*ctx.shape_args)
        dev = x.device
        grad_out = grad_out.contiguous()
        if grad_out.dtype != torch.float32:
            grad_out = grad_out.float()
        # parameter gradients: all ten or none (an attack freezes the parameters: the data-gradient chain alone)
        want_params = any(ctx.needs_input_grad[3:])
        want_dx = ctx.needs_input_grad[0]     # (only with MinimalStem.input_grad: `bn_fusable` sends any other such input elsewhere)
        ws = ctx.ws
        with torch.cuda.device(dev):
            grads = [torch.empty_like(p) for p in ps] if want_params or not want_dx else None
            d_x = torch.empty_like(x) if want_dx else None
            _lib.check(lib.node_bnministem_bwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), grad_out.data_ptr(),
                                               C.byref(_struct(grads)) if grads is not None else None,
                                               d_x.data_ptr() if d_x is not None else None, workspace.aligned_ptr(ws), ctx.nbytes,
                                               torch.cuda.current_stream(dev).cuda_stream))
        _BN_FREE.give(ctx.key, ws)       # free for the next forward of this shape (stream-ordered behind this backward)
        ctx.ws = None
        if grads is None:
            grads = [None] * len(ps)
        return (d_x, None, None, *grads)


def _hooked(seq):
    """a forward or backward hook on one of the stem's sub-modules: the node would not call it (hooks on the stem itself run)"""
    return any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, '_backward_pre_hooks', None)
               for m in seq.modules() if m is not seq)


def bn_fusable(seq, x, input_grad=False) -> bool:
    """What node_bnministem_fwd takes: an fp32 NCHW batch on a HIP device; a stem `_bn_params_of` recognises, fp32 parameters on
    the input's device, 16-byte aligned tensors, no hooks on the stem's sub-modules; an input that requires a gradient only with
    `input_grad`; no stream capture; a shape node_bnministem_workspace_bytes accepts (in_ch <= 3, filters a power of two in
    [64, 4096], h, w >= 10, tensors under 2^31 elements).  Anything else runs the module sequence."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1):
        return False
    ps = _bn_params_of(seq)
    if ps is None or ps[0].shape[1] != x.shape[1] or _hooked(seq):
        return False
    if x.requires_grad and torch.is_grad_enabled() and not input_grad:
        return False
    if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device and p.data_ptr() % 16 == 0 for p in ps):
        return False
    if x.data_ptr() % 16 or torch.cuda.is_current_stream_capturing():
        return False
    n, cin, h, w = x.shape
    shape = _lib.NodeMiniStemShape(n, cin, h, w, ps[-1].shape[0], seq[1].eps)
    return _lib.load().node_bnministem_workspace_bytes(C.byref(shape), 1) != 0      # (0: refused, with a message)


class MinimalStem(nn.Sequential):
    """`nn.Sequential(Conv2d(in_ch, 24, 3, 1), GN, ReLU, Conv2d(24, 24, 4, 2, 1), GN, ReLU, Conv2d(24, out_ch, 4, 2, 1))` with
    the reference's state_dict keys; on a HIP device its forward and backward are the library's (one autograd node).

    `input_grad` (default False): with it on, an input that requires a gradient stays on the fused path and the backward
    returns the image's gradient too (with frozen parameters only the data-gradient chain runs).  Off, such an input runs the
    module sequence.  `nof.attack.bim` switches it on for the attack's duration."""

    input_grad = False
    # norm='batch' stems as one node of the HIP library (`_BnMiniStemFn`, csrc/bnministem_api.hip) when True; False: the module
    # sequence, as before that node existed.  It ships False: at [128, 3, 32, 32] -> 256 the node's forward + backward measured
    # SLOWER than the modules (profiles/bnministem_time.txt: the reused 24-channel weight and data gradients cost more than MIOpen's
    # there), while its forward and its image gradient are faster.  `MinimalStem.fused_batch = True`, on the class or an instance,
    # switches the node on (inference, attacks, small batches).  GroupNorm stems do not read it.  `eval()` changes nothing: without
    # running statistics the reference normalises with the batch's statistics in evaluation too.
    fused_batch = False

    def forward(self, x):
        if len(self) > 1 and isinstance(self[1], nn.BatchNorm2d):
            if not (self.fused_batch and bn_fusable(self, x, self.input_grad)):
                return super().forward(x)
            ps = _bn_params_of(self)
            keep = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))
            if not keep:
                ps = [p.detach() for p in ps]
            return _BnMiniStemFn.apply(x, float(self[1].eps), keep, *ps)
        if not fusable(self, x, self.input_grad):
            return super().forward(x)
        ps = _params_of(self)
        want_x = x.requires_grad and torch.is_grad_enabled()
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in ps)):
            return _MiniStemFn.apply(x, float(self[1].eps), want_x, *[p.detach() for p in ps])
        return _MiniStemFn.apply(x, float(self[1].eps), True, *ps)

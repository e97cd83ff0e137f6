"""The residual stem in front of the ODE block -- `ResDownsample`, `/root/reference/model.py:167-178`, built from
`ResBlock` (`model.py:284-310`) -- forward and backward through the HIP library (`node_stem_fwd / node_stem_bwd`,
csrc/kernels_stem.hip): ONE autograd node for the whole stem, NHWC inside, no MIOpen call, no layout transposes, no
PyTorch reductions.  The module keeps the reference's sub-modules as parameter containers (same state_dict keys:
`0.weight`, `1.norm1.weight`, `1.conv1.weight`, `1.downsample.weight`, ...), so checkpoints load unchanged; CPU
tensors, non-fp32 inputs and geometries the kernels do not take run the plain module sequence (what the CPU baseline
and the gloo tests use) -- on a HIP device with the library missing, the fused path raises.

Images of more than 2400 pixels behind the first layer -- 64x64 inputs: tiny-imagenet-200, CIFAR-10 resized for the transfer
evaluation -- are ONE node too: `_BandedStemFn` (`node_stem_banded_fwd / node_stem_banded_bwd`), the same plan with the GroupNorm
passes that do not fit the LDS run in bands of pixels (csrc/kernels_stem_banded.hip).

A stem built with `norm='batch'` (`nn.BatchNorm2d(C, track_running_stats=False)` in the four norm slots) is ONE node as well:
`_BnStemFn` (`node_bnstem_fwd / node_bnstem_bwd`, csrc/bnstem_api.hip), the same launch plan around the BatchNorm passes of the
batch-norm dynamics.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, workspace

_WS = workspace.Carried(keep=1)      # (device, shape) -> the workspace whose backward has run


def _params_of(seq):
    """The sixteen tensors of the stem in node_stem_params order, or None if `seq` is not the reference's layout."""
    try:
        c0, b1, b2 = seq[0], seq[1], seq[2]
        ps = [c0.weight, c0.bias,
              b1.norm1.weight, b1.norm1.bias, b1.conv1.weight, b1.norm2.weight, b1.norm2.bias, b1.conv2.weight, b1.downsample.weight,
              b2.norm1.weight, b2.norm1.bias, b2.conv1.weight, b2.norm2.weight, b2.norm2.bias, b2.conv2.weight, b2.downsample.weight]
    except (AttributeError, IndexError, TypeError):
        return None
    if any(p is None for p in ps):
        return None
    for gn in (b1.norm1, b1.norm2, b2.norm1, b2.norm2):
        if not isinstance(gn, nn.GroupNorm) or gn.num_groups != min(32, gn.num_channels) or gn.eps != b1.norm1.eps:
            return None
    if c0.kernel_size != (3, 3) or c0.stride != (1, 1) or c0.padding != (0, 0) or c0.out_channels != 64:
        return None
    for blk, cin in ((b1, 64), (b2, 64)):
        if (blk.conv1.kernel_size, blk.conv1.stride, blk.conv1.padding, blk.conv1.bias) != ((3, 3), (2, 2), (1, 1), None):
            return None
        if (blk.conv2.kernel_size, blk.conv2.stride, blk.conv2.padding, blk.conv2.bias) != ((3, 3), (1, 1), (1, 1), None):
            return None
        ds = blk.downsample
        if not isinstance(ds, nn.Conv2d) or (ds.kernel_size, ds.stride, ds.padding, ds.bias) != ((1, 1), (2, 2), (0, 0), None):
            return None
        if blk.conv1.in_channels != cin:
            return None
    if b1.conv1.out_channels != 64 or b2.conv1.out_channels != b2.conv2.out_channels:
        return None
    return ps


def _bn_params_of(seq):
    """The same sixteen tensors for a `norm='batch'` stem, or None: the reference's layout with four
    `nn.BatchNorm2d(C, track_running_stats=False)` (model.py:274) -- affine, no running buffers (they would have to be updated in
    training and USED in evaluation: the node does neither), one eps -- and the convolution geometry `_params_of` asks for."""
    try:
        c0, b1, b2 = seq[0], seq[1], seq[2]
        norms = (b1.norm1, b1.norm2, b2.norm1, b2.norm2)
        ps = [c0.weight, c0.bias,
              b1.norm1.weight, b1.norm1.bias, b1.conv1.weight, b1.norm2.weight, b1.norm2.bias, b1.conv2.weight, b1.downsample.weight,
              b2.norm1.weight, b2.norm1.bias, b2.conv1.weight, b2.norm2.weight, b2.norm2.bias, b2.conv2.weight, b2.downsample.weight]
    except (AttributeError, IndexError, TypeError):
        return None
    if any(p is None for p in ps):
        return None
    for bn, c in zip(norms, (64, 64, 64, b2.conv1.out_channels)):
        if not isinstance(bn, nn.BatchNorm2d) or not bn.affine or bn.track_running_stats or bn.running_mean is not None \
                or bn.eps != b1.norm1.eps or bn.num_features != c:
            return None
    if not isinstance(c0, nn.Conv2d) or c0.kernel_size != (3, 3) or c0.stride != (1, 1) or c0.padding != (0, 0) or c0.out_channels != 64:
        return None
    for blk in (b1, b2):
        if (blk.conv1.kernel_size, blk.conv1.stride, blk.conv1.padding, blk.conv1.bias) != ((3, 3), (2, 2), (1, 1), None):
            return None
        if (blk.conv2.kernel_size, blk.conv2.stride, blk.conv2.padding, blk.conv2.bias) != ((3, 3), (1, 1), (1, 1), None):
            return None
        ds = blk.downsample
        if not isinstance(ds, nn.Conv2d) or (ds.kernel_size, ds.stride, ds.padding, ds.bias) != ((1, 1), (2, 2), (0, 0), None):
            return None
        if blk.conv1.in_channels != 64:
            return None
    if b1.conv1.out_channels != 64 or b2.conv1.out_channels != b2.conv2.out_channels:
        return None
    return ps


def _struct(tensors):
    return _lib.NodeStemParams(*[t.data_ptr() for t in tensors])


class _StemFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps, *params):
        lib = _lib.load()
        x = x.detach().contiguous()
        n, cin, h, w = x.shape
        filters = params[-1].shape[0]
        shape = _lib.NodeStemShape(n, cin, h, w, filters, eps)
        dev = x.device
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            nbytes = lib.node_stem_workspace_bytes(C.byref(shape))
            if nbytes == 0:
                _lib.unsupported()
            # the workspace carries the forward's activations to the backward: one per (device, shape) in flight (two
            # models, gradient accumulation over stems: workspace.Carried)
            key = (dev.index, n, cin, h, w, filters)
            ws = _WS.take(key, dev, nbytes)
            h2 = ((h - 2 - 1) // 2 + 1 - 1) // 2 + 1
            w2 = ((w - 2 - 1) // 2 + 1 - 1) // 2 + 1
            out = torch.empty(n, filters, h2, w2, dtype=torch.float32, device=dev)
            wsp = workspace.aligned_ptr(ws)
            _lib.check(lib.node_stem_fwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), out.data_ptr(), wsp, nbytes,
                                         torch.cuda.current_stream(dev).cuda_stream))
        ctx.shape_args = (n, cin, h, w, filters, eps)
        ctx.ws, ctx.nbytes, ctx.key = ws, nbytes, key
        ctx.save_for_backward(x, *ps)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        x, *ps = ctx.saved_tensors
        if ctx.ws is None:
            raise RuntimeError('the fused stem keeps its activations in a workspace that the first backward releases: '
                               'a second backward through the same forward (retain_graph=True) is not supported')
        shape = _lib.NodeStemShape(*ctx.shape_args)
        dev = x.device
        grad_out = grad_out.contiguous()
        # parameter gradients: all sixteen or none (an attack freezes the parameters: the data-gradient chain alone)
        want_params = any(ctx.needs_input_grad[2:])
        want_dx = ctx.needs_input_grad[0]     # (only with ResidualStem.input_grad: `fusable` sends any other such input elsewhere)
        grads = [torch.empty_like(p) for p in ps] if want_params or not want_dx else None
        ws = ctx.ws
        d_x = None
        with torch.cuda.device(dev):
            wsp = workspace.aligned_ptr(ws)
            stream = torch.cuda.current_stream(dev).cuda_stream
            if want_dx:
                d_x = torch.empty_like(x)
                _lib.check(lib.node_stem_bwd_dx(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), grad_out.data_ptr(),
                                                C.byref(_struct(grads)) if grads is not None else None, d_x.data_ptr(), wsp,
                                                ctx.nbytes, stream))
            else:
                _lib.check(lib.node_stem_bwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), grad_out.data_ptr(),
                                             C.byref(_struct(grads)), wsp, ctx.nbytes, stream))
        _WS.give(ctx.key, ws)        # free for the next forward of this shape (stream-ordered behind this backward)
        ctx.ws = None
        if grads is None:
            grads = [None] * len(ps)
        return (d_x, None, *grads)


_BANDED_WS = workspace.Carried(keep=1)      # (device, shape) -> the banded node's workspace whose backward has run


class _BandedStemFn(torch.autograd.Function):
    """`_StemFn` on node_stem_banded_fwd / node_stem_banded_bwd / node_stem_banded_bwd_dx: the stem on images past the resident
    GroupNorm passes' 2400 pixels.  Same workspace discipline (its own pool), same one-backward rule."""

    @staticmethod
    def forward(ctx, x, eps, *params):
        lib = _lib.load()
        x = x.detach().contiguous()
        n, cin, h, w = x.shape
        filters = params[-1].shape[0]
        shape = _lib.NodeStemShape(n, cin, h, w, filters, eps)
        dev = x.device
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            nbytes = lib.node_stem_banded_workspace_bytes(C.byref(shape))
            if nbytes == 0:
                _lib.unsupported()
            key = (dev.index, n, cin, h, w, filters)
            ws = _BANDED_WS.take(key, dev, nbytes)
            out = torch.empty(n, filters, _out_size(h), _out_size(w), dtype=torch.float32, device=dev)
            wsp = workspace.aligned_ptr(ws)
            _lib.check(lib.node_stem_banded_fwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), out.data_ptr(), wsp, nbytes,
                                                torch.cuda.current_stream(dev).cuda_stream))
        ctx.shape_args = (n, cin, h, w, filters, eps)
        ctx.ws, ctx.nbytes, ctx.key = ws, nbytes, key
        ctx.save_for_backward(x, *ps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if ctx.ws is None:
            raise RuntimeError('the fused stem keeps its activations in a workspace that the first backward releases: '
                               'a second backward through the same forward (retain_graph=True) is not supported')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ResidualStem: the fused backward does not run inside a stream capture')
        lib = _lib.load()
        x, *ps = ctx.saved_tensors
        shape = _lib.NodeStemShape(*ctx.shape_args)
        dev = x.device
        grad_out = grad_out.contiguous()
        if grad_out.dtype != torch.float32:
            grad_out = grad_out.float()
        if grad_out.data_ptr() % 16:
            grad_out = grad_out.clone()
        # parameter gradients: all sixteen or none (an attack freezes the parameters: the data-gradient chain alone)
        want_params = any(ctx.needs_input_grad[2:])
        want_dx = ctx.needs_input_grad[0]     # (only with ResidualStem.input_grad: `banded_fusable` sends any other such input elsewhere)
        ws = ctx.ws
        d_x = None
        with torch.cuda.device(dev):
            grads = [torch.empty_like(p) for p in ps] if want_params or not want_dx else None
            wsp = workspace.aligned_ptr(ws)
            stream = torch.cuda.current_stream(dev).cuda_stream
            if want_dx:
                d_x = torch.empty_like(x)
                _lib.check(lib.node_stem_banded_bwd_dx(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), grad_out.data_ptr(),
                                                       C.byref(_struct(grads)) if grads is not None else None, d_x.data_ptr(), wsp,
                                                       ctx.nbytes, stream))
            else:
                _lib.check(lib.node_stem_banded_bwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), grad_out.data_ptr(),
                                                    C.byref(_struct(grads)), wsp, ctx.nbytes, stream))
        _BANDED_WS.give(ctx.key, ws)        # free for the next forward of this shape (stream-ordered behind this backward)
        ctx.ws = None
        if grads is None:
            grads = [None] * len(ps)
        return (d_x, None, *grads)


def _out_size(h):
    return ((h - 2 - 1) // 2 + 1 - 1) // 2 + 1


_BN_FREE = workspace.Carried()       # (device, shape) -> workspaces whose backward has run: free for the next forward of that shape
_BN_SCRATCH = workspace.Scratch()    # (device, stream, shape) -> the workspace of forwards that keep nothing


class _BnStemFn(torch.autograd.Function):
    """The `norm='batch'` residual stem: node_bnstem_fwd / node_bnstem_bwd (csrc/bnstem_api.hip), with `resnet._BnTrunkFn`'s
    workspace discipline: a forward that wants gradients keeps its activations in a workspace of its own until its backward has
    run, a no-grad forward uses the stream's scratch and touches none of them."""

    @staticmethod
    def forward(ctx, x, eps, keep, *params):
        lib = _lib.load()
        x = x.detach().contiguous()
        n, cin, h, w = x.shape
        filters = params[-1].shape[0]
        shape_args = (n, cin, h, w, filters, eps)
        shape = _lib.NodeStemShape(*shape_args)
        dev = x.device
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            nbytes = lib.node_bnstem_workspace_bytes(C.byref(shape), 1 if keep else 0)
            if nbytes == 0:
                _lib.unsupported()
            if keep:
                key = (dev.index,) + shape_args
                ws = _BN_FREE.take(key, dev, nbytes)
            else:
                ws = _BN_SCRATCH.take(dev, nbytes, *shape_args)
            out = torch.empty(n, filters, _out_size(h), _out_size(w), dtype=torch.float32, device=dev)
            _lib.check(lib.node_bnstem_fwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), out.data_ptr(), 1 if keep else 0,
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
            raise RuntimeError('ResidualStem: the fused backward does not run inside a stream capture')
        lib = _lib.load()
        x, *ps = ctx.saved_tensors
        shape = _lib.NodeStemShape(*ctx.shape_args)
        dev = x.device
        grad_out = grad_out.contiguous()
        if grad_out.dtype != torch.float32:
            grad_out = grad_out.float()
        if grad_out.data_ptr() % 16:
            grad_out = grad_out.clone()
        # parameter gradients: all sixteen or none (an attack freezes the parameters: the data-gradient chain alone)
        want_params = any(ctx.needs_input_grad[3:])
        want_dx = ctx.needs_input_grad[0]     # (only with ResidualStem.input_grad: `bn_fusable` sends any other such input elsewhere)
        ws = ctx.ws
        with torch.cuda.device(dev):
            grads = [torch.empty_like(p) for p in ps] if want_params or not want_dx else None
            d_x = torch.empty_like(x) if want_dx else None
            _lib.check(lib.node_bnstem_bwd(C.byref(shape), C.byref(_struct(ps)), x.data_ptr(), grad_out.data_ptr(),
                                           C.byref(_struct(grads)) if grads is not None else None,
                                           d_x.data_ptr() if want_dx else None, workspace.aligned_ptr(ws), ctx.nbytes,
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


def _is_batch(seq):
    """the first norm is a BatchNorm2d (one look, so that GroupNorm stems pay nothing for the other node)"""
    return len(seq) > 1 and isinstance(getattr(seq[1], 'norm1', None), nn.BatchNorm2d)


def bn_fusable(seq, x, input_grad=False) -> bool:
    """What node_bnstem_fwd takes: an fp32 NCHW batch on a HIP device with in_ch <= 3, h, w >= 5 and up to 2400 pixels behind the
    first layer; a stem `_bn_params_of` recognises, filters a multiple of 64 in [64, 4096] (192 and 384 included), fp32 parameters
    on the input's device, 16-byte aligned tensors under 2^31 elements, no hooks on the stem's sub-modules; more than one value
    per channel at the last norm (N H2 W2 = 1 is what nn.BatchNorm2d refuses: the modules raise it); an input that requires a
    gradient only with `input_grad`; no stream capture.  Anything else runs the module sequence."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and 1 <= x.shape[1] <= 3 and x.shape[0] >= 1
            and min(x.shape[2], x.shape[3]) >= 5 and (x.shape[2] - 2) * (x.shape[3] - 2) <= 2400):
        return False
    ps = _bn_params_of(seq)
    if ps is None or _hooked(seq):
        return False
    if x.requires_grad and torch.is_grad_enabled() and not input_grad:
        return False
    n, cin, h, w = x.shape
    filters = ps[-1].shape[0]
    if not (filters % 64 == 0 and 64 <= filters <= 4096 and ps[0].shape[1] == cin and n * _out_size(h) * _out_size(w) > 1
            and (n * (h - 2) * (w - 2) + 1) * 64 < 2 ** 31 and (n * _out_size(h) * _out_size(w) + 1) * filters < 2 ** 31):
        return False
    if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device and p.data_ptr() % 16 == 0 for p in ps):
        return False
    return x.data_ptr() % 16 == 0 and not torch.cuda.is_current_stream_capturing()


def fusable(seq, x, input_grad=False) -> bool:
    """What the library's stem kernels take (node_stem_fwd): fp32 on a HIP device, in_ch <= 3, filters a power of two >= 64,
    images of up to 2400 pixels behind the first layer (the GroupNorm passes hold a (sample, 8 channels) block in LDS).
    Larger images -- 64x64 inputs -- are `banded_fusable`'s; anything else -- the 24- and 32-filter toy nets of the tests --
    runs the module sequence."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] <= 3
            and min(x.shape[2], x.shape[3]) >= 5 and (x.shape[2] - 2) * (x.shape[3] - 2) <= 2400):
        return False
    ps = _params_of(seq)
    if x.requires_grad and torch.is_grad_enabled() and not input_grad:
        # by default the fused backward produces parameter gradients only (saliency / adversarial inputs: module sequence);
        # ResidualStem.input_grad opts in to node_stem_bwd_dx, which also returns the image's gradient
        return False
    filters = ps[-1].shape[0] if ps is not None else 0
    # power-of-two filter counts: the GroupNorm passes keep whole groups inside power-of-two channel blocks (192, 384, ... are
    # refused by check_stem_shape, csrc/stem_api.hip)
    return (ps is not None and filters % 64 == 0 and filters & (filters - 1) == 0 and ps[0].shape[1] == x.shape[1]
            and all(p.is_cuda and p.dtype == torch.float32 for p in ps))


def banded_fusable(seq, x, input_grad=False) -> bool:
    """What node_stem_banded_fwd takes: `fusable`'s conditions without the pixel ceiling -- an fp32 NCHW batch on a HIP device,
    n >= 1, in_ch <= 3, h, w >= 5; a stem `_params_of` recognises with filters a power of two in [64, 4096], fp32 parameters on the
    input's device; an input that requires a gradient only with `input_grad` -- and on top of them: every tensor of the plan under
    2^31 elements, 16-byte aligned tensors, no hooks on the stem's sub-modules (the node would not call them), no stream capture.
    Anything else runs the module sequence."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and 1 <= x.shape[1] <= 3 and x.shape[0] >= 1
            and min(x.shape[2], x.shape[3]) >= 5):
        return False
    ps = _params_of(seq)
    if ps is None or _hooked(seq):
        return False
    if x.requires_grad and torch.is_grad_enabled() and not input_grad:
        return False
    n, cin, h, w = x.shape
    filters = ps[-1].shape[0]
    h1, w1 = (h - 2 - 1) // 2 + 1, (w - 2 - 1) // 2 + 1
    if not (64 <= filters <= 4096 and filters & (filters - 1) == 0 and ps[0].shape[1] == cin
            and (n * (h - 2) * (w - 2) + 1) * 64 < 2 ** 31 and (n * h1 * w1 + 1) * 64 < 2 ** 31
            and (n * _out_size(h) * _out_size(w) + 1) * filters < 2 ** 31 and n * cin * h * w < 2 ** 31):
        return False
    if not all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device and p.data_ptr() % 16 == 0 for p in ps):
        return False
    return x.data_ptr() % 16 == 0 and not torch.cuda.is_current_stream_capturing()


class ResidualStem(nn.Sequential):
    """`nn.Sequential(Conv2d(in_ch, 64, 3, 1), ResBlock(64, 64, 2, conv1x1), ResBlock(64, out_ch, 2, conv1x1))` with the
    reference's state_dict keys; on a HIP device its forward and backward are the library's (one autograd node).

    `input_grad` (default False): with it on, an input that requires a gradient stays on the fused path and the backward
    returns the image's gradient too (node_stem_bwd_dx; with frozen parameters only the data-gradient chain runs).  Off, such
    an input runs the module sequence, as it always has.  `nof.attack.bim` switches it on for the attack's duration."""

    input_grad = False
    # norm='batch' stems as one node of the HIP library (`_BnStemFn`, csrc/bnstem_api.hip); False: the module sequence, as before that
    # node existed (A/B runs, tests).  GroupNorm stems do not read it.  `eval()` changes nothing: without running statistics the
    # reference normalises with the batch's statistics in evaluation too.
    fused_batch = True
    # GroupNorm stems on images past the resident passes' 2400 pixels (64x64 inputs) as one node (`_BandedStemFn`,
    # node_stem_banded_*); False: the module sequence, as before that node existed (A/B runs, tests).  Shapes `fusable` takes never
    # read it.
    fused_banded = True

    def forward(self, x):
        if _is_batch(self) and self.fused_batch and bn_fusable(self, x, self.input_grad):
            ps = _bn_params_of(self)
            keep = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))
            if not keep:
                ps = [p.detach() for p in ps]
            return _BnStemFn.apply(x, float(self[1].norm1.eps), keep, *ps)
        if fusable(self, x, self.input_grad):
            fn = _StemFn
        elif self.fused_banded and banded_fusable(self, x, self.input_grad):
            fn = _BandedStemFn
        else:
            return super().forward(x)
        ps = _params_of(self)
        if not (torch.is_grad_enabled() and any(p.requires_grad for p in ps)):
            return fn.apply(x, float(self[1].norm1.eps), *[p.detach() for p in ps])
        return fn.apply(x, float(self[1].norm1.eps), *ps)

"""The ResNet baseline of the reference (`model.py:65-111`): stem -> six `ResBlock(C, C)` -> classifier head.  Every
comparison the reference makes is ODENet against this net (`reproduce.sh` trains it first, `utils.py:262-265` builds it
for every run that is not an `odenet`, `evaluate.py:65-67` reads seven "time points" from it: the stem's output and the
outputs of its six blocks).

`ResidualTrunk` is the `features` member: an `nn.Sequential` of the package's `ResBlock`s (the reference's state_dict
keys, `features.<i>.norm1.weight`, ...) whose forward and backward on a HIP device are ONE autograd node through the
library (`node_trunk_fwd / node_trunk_bwd`, csrc/trunk_api.hip): the stem's gather-GEMM convolutions on bf16 triples,
the residual added in the second convolution's epilogue, NHWC inside, no MIOpen call, no layout transposes.  A `norm='batch'`
trunk (`train --model resnet --norm batch`, the net every ODE-Net comparison of the reference is made against) is the same plan
around the BatchNorm passes of the batch-norm dynamics (`node_bntrunk_fwd / node_bntrunk_bwd`, csrc/bntrunk_api.hip).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, workspace
from .odenet import FCClassifier, ResBlock, _Wrapped, _stem, head_on_trajectory

def _block_params(blk):
    return [blk.norm1.weight, blk.norm1.bias, blk.conv1.weight, blk.norm2.weight, blk.norm2.bias, blk.conv2.weight]


def _norm_form(norm):
    """'group' / 'batch' for the two norms the library's trunks take, None for anything else: the reference's
    GroupNorm(min(32, C), C), or its BatchNorm2d(C, track_running_stats=False) (model.py:268-281), affine."""
    if isinstance(norm, nn.GroupNorm):
        return 'group' if norm.affine and norm.num_groups == min(32, norm.num_channels) else None
    if isinstance(norm, nn.BatchNorm2d):
        # running statistics would have to be updated in training and USED in evaluation: the node does neither
        return 'batch' if norm.affine and not norm.track_running_stats and norm.running_mean is None else None
    return None


def _form_of(seq):
    """(form, tensors) of a recognised trunk -- form 'group' or 'batch', the tensors six per block in node_trunk_block
    order -- or None if `seq` is not `blocks` x the reference's ResBlock(C, C) (stride 1, no downsample, 3x3 / 1 / 1
    convolutions without bias, no hooks on the blocks) with ONE of the two norms and one eps throughout."""
    blocks = list(seq.children())
    if not blocks:
        return None
    ps = []
    c = None
    eps = None
    form = None
    for blk in blocks:
        if not isinstance(blk, ResBlock) or blk.downsample is not None or blk._forward_hooks or blk._forward_pre_hooks:
            return None
        for norm in (blk.norm1, blk.norm2):
            f = _norm_form(norm)
            if f is None:
                return None
            nc = norm.num_channels if f == 'group' else norm.num_features
            form = f if form is None else form
            c = nc if c is None else c
            eps = norm.eps if eps is None else eps
            if f != form or nc != c or norm.eps != eps:
                return None
        for conv in (blk.conv1, blk.conv2):
            if (conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.bias, conv.padding_mode) != \
                    ((3, 3), (1, 1), (1, 1), (1, 1), 1, None, 'zeros') or conv.in_channels != c or conv.out_channels != c:
                return None
        ps += _block_params(blk)
    return form, ps


def _params_of(seq):
    """The trunk's tensors, six per block in node_trunk_block order, or None if `seq` is not a trunk `_form_of` recognises."""
    got = _form_of(seq)
    return None if got is None else got[1]


def _struct_array(tensors):
    n = len(tensors) // 6
    arr = (_lib.NodeTrunkBlock * n)()
    for i in range(n):
        arr[i] = _lib.NodeTrunkBlock(*[t.data_ptr() for t in tensors[6 * i:6 * i + 6]])
    return arr


class _Entry:
    """The library calls and the two workspace pools of one trunk node (the workspaces of the two norms have different layouts)."""

    def __init__(self, name):
        self.bytes, self.fwd, self.bwd = 'node_%s_workspace_bytes' % name, 'node_%s_fwd' % name, 'node_%s_bwd' % name
        self.free = workspace.Carried()       # (device, shape) -> workspaces whose backward has run: free for the next forward of that shape
        self.scratch = workspace.Scratch()    # (device, stream, shape) -> the workspace of forwards that keep nothing


_GROUP, _BATCH = _Entry('trunk'), _Entry('bntrunk')


def _node_forward(entry, ctx, x, eps, want_taps, keep, *params):
    lib = _lib.load()
    x = x.detach().contiguous()
    n, c, h, w = x.shape
    nblocks = len(params) // 6
    shape_args = (n, c, h, w, nblocks, eps)
    shape = _lib.NodeTrunkShape(*shape_args)
    dev = x.device
    ps = [p.detach().contiguous() for p in params]
    with torch.cuda.device(dev):
        nbytes = getattr(lib, entry.bytes)(C.byref(shape), 1 if keep else 0)
        if nbytes == 0:
            _lib.unsupported()
        if keep:
            # the workspace carries this forward's activations to its backward: one per forward in flight
            # (--batch-accumulation, two models: workspace.Carried)
            key = (dev.index,) + shape_args
            ws = entry.free.take(key, dev, nbytes)
        else:
            ws = entry.scratch.take(dev, nbytes, *shape_args)
        out = torch.empty_like(x)
        taps = torch.empty((nblocks,) + tuple(x.shape), dtype=torch.float32, device=dev) if want_taps else None
        _lib.check(getattr(lib, entry.fwd)(C.byref(shape), _struct_array(ps), x.data_ptr(), out.data_ptr(),
                                           taps.data_ptr() if want_taps else None, 1 if keep else 0, workspace.aligned_ptr(ws),
                                           nbytes, torch.cuda.current_stream(dev).cuda_stream))
    ctx.ws = None
    if keep:
        ctx.shape_args, ctx.ws, ctx.nbytes, ctx.key = shape_args, ws, nbytes, key
        ctx.save_for_backward(*ps)
    if want_taps:
        ctx.mark_non_differentiable(taps)
        return out, taps
    return out


def _node_backward(entry, ctx, grad_out):
    if ctx.ws is None:
        raise RuntimeError('the fused trunk keeps its activations in a workspace that the first backward releases: '
                           'a second backward through the same forward (retain_graph=True) is not supported')
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('ResidualTrunk: the fused backward does not run inside a stream capture')
    lib = _lib.load()
    ps = list(ctx.saved_tensors)
    shape = _lib.NodeTrunkShape(*ctx.shape_args)
    dev = ps[0].device
    grad_out = grad_out.contiguous()
    if grad_out.dtype != torch.float32:
        grad_out = grad_out.float()
    ws = ctx.ws
    with torch.cuda.device(dev):
        grads = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(grad_out)
        _lib.check(getattr(lib, entry.bwd)(C.byref(shape), _struct_array(ps), grad_out.data_ptr(), _struct_array(grads),
                                           dx.data_ptr(), workspace.aligned_ptr(ws), ctx.nbytes,
                                           torch.cuda.current_stream(dev).cuda_stream))
    entry.free.give(ctx.key, ws)      # free for the next forward of this shape (stream-ordered behind this backward)
    ctx.ws = None
    return (dx, None, None, None, *grads)


class _TrunkFn(torch.autograd.Function):
    """`blocks` x ResBlock(C, C) with GroupNorm: node_trunk_fwd / node_trunk_bwd (csrc/trunk_api.hip)."""

    @staticmethod
    def forward(ctx, x, eps, want_taps, keep, *params):
        return _node_forward(_GROUP, ctx, x, eps, want_taps, keep, *params)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *unused):
        return _node_backward(_GROUP, ctx, grad_out)


class _BnTrunkFn(torch.autograd.Function):
    """The same for `blocks` x ResBlock(C, C, norm='batch'): node_bntrunk_fwd / node_bntrunk_bwd (csrc/bntrunk_api.hip)."""

    @staticmethod
    def forward(ctx, x, eps, want_taps, keep, *params):
        return _node_forward(_BATCH, ctx, x, eps, want_taps, keep, *params)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *unused):
        return _node_backward(_BATCH, ctx, grad_out)


def fusable(seq, x) -> bool:
    """What the library's trunks take (node_trunk_fwd, node_bntrunk_fwd): an fp32 NCHW batch on a HIP device, `blocks` x the
    reference's ResBlock(C, C), tensors under 2^31 elements, parameters fp32 on the input's device, and
      GroupNorm: C a power of two in [64, 4096], images of up to 2400 pixels (the passes hold a (sample, channel block) in LDS);
      BatchNorm (affine, no running statistics; `seq.fused_batch` not switched off): C a multiple of 64 in [64, 4096], more than
        one value per channel (N H W = 1 is what nn.BatchNorm2d refuses: the modules raise it), 16-byte aligned tensors.
    Anything else -- the 16- and 32-filter nets of the tests, C = 96, CPU tensors -- runs the module sequence."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1):
        return False
    got = _form_of(seq)
    if got is None:
        return False
    form, ps = got
    c = ps[0].shape[0]
    n, cx, h, w = x.shape
    if not (cx == c and 64 <= c <= 4096 and (n * h * w + 1) * c < 2 ** 31
            and all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in ps)):
        return False
    if form == 'group':
        return c & (c - 1) == 0 and 1 <= h * w <= 2400
    return (getattr(seq, 'fused_batch', True) and c % 64 == 0 and n * h * w > 1
            and all(p.data_ptr() % 16 == 0 for p in ps) and x.data_ptr() % 16 == 0)


class ResidualTrunk(nn.Sequential):
    """`nn.Sequential(*[ResBlock(C, C) for _ in range(blocks)])` (model.py:79) with the reference's state_dict keys.  On a
    HIP device forward and backward are one autograd node (`_TrunkFn`) through the library; it returns every parameter
    gradient and the input gradient (the stem trains behind it).  A forward that wants gradients keeps its activations
    in a workspace of its own until its backward has run, so several forwards may be in flight (gradient accumulation)
    and no-grad forwards in between touch none of them.  The first backward releases the workspace: a SECOND backward
    through the same forward (`retain_graph=True`) raises, as the fused stem's does.  A forward under stream capture with
    gradients wanted, and every input `fusable` refuses, run `nn.Sequential.forward`.  With `norm='batch'` the node is
    `_BnTrunkFn` (csrc/bntrunk_api.hip), with the same rules."""

    # norm='batch' trunks as one node of the HIP library (`_BnTrunkFn`); False: the module sequence, as before that node existed
    # (A/B runs, tests).  GroupNorm trunks do not read it.
    fused_batch = True

    def __init__(self, channels, blocks=6, norm='group'):
        super().__init__(*[ResBlock(channels, channels, norm=norm) for _ in range(blocks)])

    def _wants_grad(self, x, ps):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))

    def _fused(self, x, want_taps):
        form, ps = _form_of(self)
        keep = self._wants_grad(x, ps)
        if not keep:
            ps = [p.detach() for p in ps]
        fn = _TrunkFn if form == 'group' else _BnTrunkFn
        return fn.apply(x, float(self[0].norm1.eps), want_taps, keep, *ps)

    def _takes_fused(self, x):
        return fusable(self, x) and not (self._wants_grad(x, _params_of(self)) and torch.cuda.is_current_stream_capturing())

    def forward(self, x):
        if not self._takes_fused(x):
            return super().forward(x)
        return self._fused(x, False)

    def forward_taps(self, x):
        """(output, [every block's output]): the fused node writes them in one forward; otherwise block by block."""
        out, taps = self.forward_taps_stacked(x)
        return out, (list(taps.unbind(0)) if torch.is_tensor(taps) else taps)

    def forward_taps_stacked(self, x):
        """`forward_taps` with the taps as the fused node writes them, ONE tensor [blocks, N, C, H, W] (a trajectory for the head:
        no copy); the list of the blocks' outputs where the modules ran."""
        if self._takes_fused(x):
            return self._fused(x, True)
        taps = []
        for blk in self:
            x = blk(x)
            taps.append(x)
        return x, taps


class ResNet(nn.Module):
    """model.py:65-111: `downsample` (one of the four non-ODE stems), `features` (six residual blocks), `classifier`."""

    def __init__(self, in_ch, out=10, n_filters=64, downsample='residual', dropout=0, norm='group'):
        super().__init__()
        if downsample not in ('residual', 'convolution', 'minimal', 'one-shot'):
            raise NotImplementedError('ResNet: downsample=%r (model.py:70-77 knows residual, convolution, minimal, one-shot)' % (downsample,))
        self.downsample = _Wrapped(_stem(downsample, in_ch, n_filters, norm))
        self.features = ResidualTrunk(n_filters, 6, norm=norm)
        self.classifier = FCClassifier(n_filters, out=out, dropout=dropout, norm=norm)
        self._extract_features = False

    def to_features_extractor(self, keep_pool=True):
        """model.py:83-99: `forward` then returns the classifier (without its last layer; with `keep_pool=False` only its
        GroupNorm + ReLU) applied to the stem's output and to each block's output: [7, N, C] or [7, N, C, H, W]."""
        if keep_pool:
            self.classifier.module[-1] = nn.Sequential()
        else:
            self.classifier = nn.Sequential(*list(self.classifier.module.children())[:2])
        self._extract_features = True

    def forward(self, x):
        x = self.downsample(x)
        if self._extract_features:
            _, taps = self.features.forward_taps_stacked(x)
            if torch.is_tensor(taps):
                # the fused trunk's taps are one tensor: two head calls (stem output, taps) instead of seven, and no copy of the taps
                return torch.cat([head_on_trajectory(self.classifier, x.detach().unsqueeze(0)),
                                  head_on_trajectory(self.classifier, taps.detach())])
            return torch.stack([self.classifier(f.detach()) for f in [x] + taps])
        return self.classifier(self.features(x))

    def nfe(self, reset=False):
        return 0


def build_model(params, in_ch, out):
    """The net a run's parameters describe (`utils.load_model`, utils.py:248-270): `params` is the argparse namespace of
    `train` or the `params` dictionary of a checkpoint; a missing `model` key is an `odenet` (runs of before the flag)."""
    from .odenet import ODENet
    get = params.get if isinstance(params, dict) else lambda k, d=None: getattr(params, k, d)
    kind = get('model', 'odenet') or 'odenet'
    common = dict(out=out, n_filters=get('filters', 64), downsample=get('downsample', 'residual'), dropout=get('dropout', 0),
                  norm=get('norm', 'group'))
    if kind == 'resnet':
        return ResNet(in_ch, **common)
    if kind != 'odenet':
        raise ValueError('unknown model %r (resnet or odenet)' % (kind,))
    model = ODENet(in_ch, method=get('method', 'dopri5'), tol=get('tol', 1e-3), adjoint=get('adjoint', False), **common)
    if common['norm'] == 'batch':
        # the command lines solve batch-norm dynamics inside the library (bnsolve.py); the class default stays the generic solver
        from .modules import ODEfunc
        for m in model.modules():
            if isinstance(m, ODEfunc):
                m.batch_solve = True
    return model

"""Fused classifier head: GroupNorm -> ReLU -> global average pool -> [Dropout] -> Flatten
(`/root/reference/model.py:231-250`, FCClassifier without its Linear layer) as ONE HIP launch forward
and one backward (`node_head_fwd / node_head_bwd`, csrc/kernels_head.hip) instead of ~15 launch-bound
PyTorch kernels.  The dropout mask is drawn by PyTorch's own generator (so seeds reproduce what
`nn.Dropout` would have drawn on the pooled `[N, C, 1, 1]` tensor) and handed to the kernel as a
per-(sample, channel) scale.  No CPU or PyTorch fallback inside: callers route non-CUDA / non-fp32
inputs to the plain module sequence themselves (`FCClassifier.forward`).  The head of a `norm='batch'`
net (BatchNorm2d without running statistics in place of the GroupNorm) has kernels of its own, two
launches each way: `bn_head_pool` (`node_bnhead_fwd / node_bnhead_bwd`, csrc/kernels_bnhead.hip)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


class _HeadPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gamma, beta, scale, groups, eps):
        lib = _lib.load()
        z = z.contiguous()
        n, c, h, w = z.shape
        shape = _lib.NodeShape(n, c, h, w, groups, eps)
        pooled = torch.empty(n, c, device=z.device, dtype=torch.float32)
        stats = torch.empty(n, groups, 2, device=z.device, dtype=torch.float32)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        stream = torch.cuda.current_stream(z.device).cuda_stream
        with torch.cuda.device(z.device):
            _lib.check(lib.node_head_fwd(shape, _ptr(z), _ptr(g), _ptr(b), _ptr(scale), _ptr(pooled), _ptr(stats), stream))
        ctx.save_for_backward(z, g, b, scale, stats)
        ctx.shape = (n, c, h, w, groups, eps)
        return pooled

    @staticmethod
    def backward(ctx, g_pooled):
        lib = _lib.load()
        z, g, b, scale, stats = ctx.saved_tensors
        n, c, h, w, groups, eps = ctx.shape
        shape = _lib.NodeShape(n, c, h, w, groups, eps)
        g_pooled = g_pooled.contiguous()
        dz = torch.empty_like(z)
        gpart = torch.empty(n + 1, 2, c, device=z.device, dtype=torch.float32)     # per-sample partials, then their sums
        dgamma, dbeta = gpart[n].unbind(0)
        stream = torch.cuda.current_stream(z.device).cuda_stream
        with torch.cuda.device(z.device):
            _lib.check(lib.node_head_bwd(shape, _ptr(z), _ptr(g), _ptr(b), _ptr(scale), _ptr(stats), _ptr(g_pooled),
                                     _ptr(dz), _ptr(gpart), _ptr(dgamma), stream))
        return dz, dgamma, dbeta, None, None, None


def head_pool(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
              p: float = 0.0, training: bool = False) -> torch.Tensor:
    """pooled[n, c] = dropout(mean_px relu(GroupNorm(z)))   -- model.py:239-247."""
    scale = None
    if training and p > 0.0:
        # exactly the numbers nn.Dropout would multiply the pooled [N, C, 1, 1] tensor by
        scale = F.dropout(torch.ones(z.shape[0], z.shape[1], 1, 1, device=z.device, dtype=torch.float32), p, True)
        scale = scale.reshape(z.shape[0], z.shape[1]).contiguous()
    return _HeadPool.apply(z, gamma, beta, scale, groups, eps)


class _BnHeadPool(torch.autograd.Function):
    """The same head behind `nn.BatchNorm2d(C, track_running_stats=False)` (model.py:274): statistics across the batch, so a kernel
    family of its own (`node_bnhead_fwd / node_bnhead_bwd`, csrc/kernels_bnhead.hip), two launches each way."""

    @staticmethod
    def forward(ctx, z, gamma, beta, scale, eps):
        lib = _lib.load()
        z = z.contiguous()
        n, c, h, w = z.shape
        shape = _lib.NodeBnfuncShape(n, c, h, w, eps)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        stream = torch.cuda.current_stream(z.device).cuda_stream
        with torch.cuda.device(z.device):
            nbytes = lib.node_bnhead_scratch_bytes(shape)
            if nbytes == 0:
                _lib.unsupported()
            pooled = torch.empty(n, c, device=z.device, dtype=torch.float32)
            stats = torch.empty(2, c, device=z.device, dtype=torch.float32)
            scratch = torch.empty(nbytes // 8, device=z.device, dtype=torch.float64)
            _lib.check(lib.node_bnhead_fwd(shape, _ptr(z), _ptr(g), _ptr(b), _ptr(scale), _ptr(pooled), _ptr(stats), _ptr(scratch), stream))
        ctx.save_for_backward(z, g, b, scale, stats)
        ctx.shape = (n, c, h, w, eps)
        return pooled

    @staticmethod
    def backward(ctx, g_pooled):
        lib = _lib.load()
        z, g, b, scale, stats = ctx.saved_tensors
        n, c, h, w, eps = ctx.shape
        shape = _lib.NodeBnfuncShape(n, c, h, w, eps)
        g_pooled = g_pooled.contiguous()
        if g_pooled.dtype != torch.float32:
            g_pooled = g_pooled.float()
        stream = torch.cuda.current_stream(z.device).cuda_stream
        with torch.cuda.device(z.device):
            dz = torch.empty_like(z)
            dgb = torch.empty(2, c, device=z.device, dtype=torch.float32)
            dgamma, dbeta = dgb.unbind(0)
            scratch = torch.empty(lib.node_bnhead_scratch_bytes(shape) // 8, device=z.device, dtype=torch.float64)
            _lib.check(lib.node_bnhead_bwd(shape, _ptr(z), _ptr(g), _ptr(b), _ptr(scale), _ptr(stats), _ptr(g_pooled), _ptr(dz),
                                           _ptr(dgamma), _ptr(dbeta), _ptr(scratch), stream))
        return dz, dgamma, dbeta, None, None


def bn_head_fusable(z: torch.Tensor, norm) -> bool:
    """What `bn_head_pool` takes: an fp32 NCHW batch on a HIP device in front of an affine `nn.BatchNorm2d` without running
    statistics, C a multiple of 64 in [64, 4096], more than one value per channel (N H W = 1 is what nn.BatchNorm2d itself refuses:
    the module raises it), tensors under 2^31 elements."""
    if not (isinstance(norm, torch.nn.BatchNorm2d) and norm.affine and not norm.track_running_stats and norm.running_mean is None
            and not norm._forward_hooks and not norm._forward_pre_hooks):
        return False
    if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and z.shape[0] >= 1):
        return False
    n, c, h, w = z.shape
    return (c == norm.num_features and c % 64 == 0 and 64 <= c <= 4096 and n * h * w > 1 and z.numel() < 2 ** 31
            and all(p.is_cuda and p.dtype == torch.float32 and p.device == z.device for p in (norm.weight, norm.bias)))


def bn_head_pool(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, p: float = 0.0,
                 training: bool = False) -> torch.Tensor:
    """pooled[n, c] = dropout(mean_px relu(BatchNorm(z))), batch statistics   -- model.py:239-247 with model.py:274."""
    scale = None
    if training and p > 0.0:
        # exactly the numbers nn.Dropout would multiply the pooled [N, C, 1, 1] tensor by (as head_pool draws them)
        scale = F.dropout(torch.ones(z.shape[0], z.shape[1], 1, 1, device=z.device, dtype=torch.float32), p, True)
        scale = scale.reshape(z.shape[0], z.shape[1]).contiguous()
    return _BnHeadPool.apply(z, gamma, beta, scale, eps)


class _GnRelu(torch.autograd.Function):
    """out = [relu](GroupNorm(z)) -- the stem's `relu(norm(x))` pairs (model.py:304-307), one launch each way."""

    @staticmethod
    def forward(ctx, z, gamma, beta, groups, eps, relu):
        lib = _lib.load()
        z = z.contiguous()
        n, c, h, w = z.shape
        shape = _lib.NodeShape(n, c, h, w, groups, eps)
        out = torch.empty_like(z)
        stats = torch.empty(n, groups, 2, device=z.device, dtype=torch.float32)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        stream = torch.cuda.current_stream(z.device).cuda_stream
        with torch.cuda.device(z.device):
            _lib.check(lib.node_gn_relu_fwd(shape, _ptr(z), _ptr(g), _ptr(b), int(relu), _ptr(out), _ptr(stats), stream))
        ctx.save_for_backward(z, g, b, stats)
        ctx.shape = (n, c, h, w, groups, eps, int(relu))
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.load()
        z, g, b, stats = ctx.saved_tensors
        n, c, h, w, groups, eps, relu = ctx.shape
        shape = _lib.NodeShape(n, c, h, w, groups, eps)
        g_out = g_out.contiguous()
        dz = torch.empty_like(z)
        gpart = torch.empty(n + 1, 2, c, device=z.device, dtype=torch.float32)     # per-sample partials, then their sums
        dgamma, dbeta = gpart[n].unbind(0)
        stream = torch.cuda.current_stream(z.device).cuda_stream
        with torch.cuda.device(z.device):
            _lib.check(lib.node_gn_relu_bwd(shape, _ptr(z), _ptr(g), _ptr(b), _ptr(stats), relu, _ptr(g_out), _ptr(dz),
                                        _ptr(gpart), _ptr(dgamma), stream))
        return dz, dgamma, dbeta, None, None, None


def gn_relu(z: torch.Tensor, norm: torch.nn.GroupNorm, relu: bool = True) -> torch.Tensor:
    """`relu(norm(z))` for CUDA fp32 4-D inputs through the fused HIP kernels; the plain modules otherwise."""
    if z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and isinstance(norm, torch.nn.GroupNorm) and norm.affine:
        return _GnRelu.apply(z, norm.weight, norm.bias, norm.num_groups, norm.eps, relu)
    out = norm(z)
    return F.relu(out) if relu else out


# ---------------------------------------------------------------------------------------------------------------
# Linear + cross-entropy (model.py:244-250 `nn.Linear(in_ch, out)`, train.py:43 `F.cross_entropy(p, y)`): one launch each
# way (node_head_loss_fwd / node_head_loss_bwd, csrc/kernels_loss.hip) instead of 3 hipBLASLt + ~10 ATen launches.
# ---------------------------------------------------------------------------------------------------------------
import ctypes as C

_LOSS_SCRATCH = {}
_LINEAR_ATTR = '_node_linear_inputs'         # on a logits tensor: the (pooled, weight, bias) `linear` computed it from


def _scratch(device, n):
    """Partials + arrival counter of the loss reduction: zero before the first use, left at zero by every launch; one per
    (device, stream)."""
    lib = _lib.load()
    need = lib.node_head_loss_scratch_bytes(int(n)) // 4
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _LOSS_SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.zeros(max(need, 1024), dtype=torch.float32, device=device)
        _LOSS_SCRATCH[key] = buf
    return buf


def _loss_struct(n, c, classes, reduction, pooled=None, weight=None, bias=None, target=None, logits=None, loss=None,
                 stat=None, scratch=None):
    return _lib.NodeHeadLoss(n, c, classes, reduction, _ptr(pooled), _ptr(weight), _ptr(bias), _ptr(target), _ptr(logits),
                             _ptr(loss), _ptr(stat), _ptr(scratch))


def _fusable_linear(x, weight, bias):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and weight.is_cuda and weight.dtype == torch.float32
            and weight.dim() == 2 and weight.shape[1] == x.shape[1] and weight.shape[0] <= 1024
            and (bias is None or (bias.is_cuda and bias.dtype == torch.float32)))


class _Linear(torch.autograd.Function):
    """logits = pooled @ W^T + b (one launch); backward from a given dL/dlogits (one launch)."""

    @staticmethod
    def forward(ctx, pooled, weight, bias):
        lib = _lib.load()
        p, w = pooled.detach().contiguous(), weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        n, c = p.shape
        o = w.shape[0]
        logits = torch.empty(n, o, dtype=torch.float32, device=p.device)
        with torch.cuda.device(p.device):
            _lib.check(lib.node_head_loss_fwd(C.byref(_loss_struct(n, c, o, 0, pooled=p, weight=w, bias=b, logits=logits)),
                                              torch.cuda.current_stream(p.device).cuda_stream))
        ctx.save_for_backward(p, w)
        ctx.has_bias = bias is not None
        return logits

    @staticmethod
    def backward(ctx, g_logits):
        lib = _lib.load()
        p, w = ctx.saved_tensors
        n, c = p.shape
        o = w.shape[0]
        g = g_logits.contiguous()
        dp, dw = torch.empty_like(p), torch.empty_like(w)
        db = torch.empty(o, dtype=torch.float32, device=p.device) if ctx.has_bias else None
        grads = _lib.NodeHeadLossGrad(None, _ptr(g), None, _ptr(dp), _ptr(dw), _ptr(db))
        with torch.cuda.device(p.device):
            _lib.check(lib.node_head_loss_bwd(C.byref(_loss_struct(n, c, o, 0, pooled=p, weight=w)), C.byref(grads),
                                              torch.cuda.current_stream(p.device).cuda_stream))
        return dp, dw, db


def linear(x: torch.Tensor, weight: torch.Tensor, bias=None) -> torch.Tensor:
    """`F.linear` for the classifier's last layer: the library's kernel for [N, C] fp32 inputs on a HIP device (at most
    1024 outputs), PyTorch's otherwise.  The result remembers what it was computed from, so that `cross_entropy` on it
    can run Linear's and the loss's backward as one launch."""
    if not _fusable_linear(x, weight, bias):
        return F.linear(x, weight, bias)
    out = _Linear.apply(x, weight, bias)
    if torch.is_grad_enabled() and out.requires_grad:
        # (with the version of the result: an in-place edit of the logits between `linear` and `cross_entropy` -- `logits.div_(T)`,
        #  `masked_fill_` -- must take the ordinary autograd edge, not the fused backward that assumes logits = x W^T + b)
        setattr(out, _LINEAR_ATTR, (x, weight, bias, out._version))
    return out


class _CrossEntropy(torch.autograd.Function):
    """loss = CE(logits, target) for given logits: one launch forward, one backward (d_logits)."""

    @staticmethod
    def forward(ctx, logits, target, reduction):
        lib = _lib.load()
        lg = logits.detach().contiguous()
        n, o = lg.shape
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        stat = torch.empty(2, dtype=torch.float32, device=lg.device)       # {loss, correct predictions}
        with torch.cuda.device(lg.device):
            h = _loss_struct(n, 0, o, reduction, target=target, logits=lg, loss=loss, stat=stat, scratch=_scratch(lg.device, n))
            _lib.check(lib.node_head_loss_fwd(C.byref(h), torch.cuda.current_stream(lg.device).cuda_stream))
        ctx.save_for_backward(lg, target)
        ctx.reduction = reduction
        ctx.mark_non_differentiable(stat)
        return loss, stat

    @staticmethod
    def backward(ctx, g_loss, _g_stat):
        lib = _lib.load()
        lg, target = ctx.saved_tensors
        n, o = lg.shape
        dl = torch.empty_like(lg)
        g = g_loss.contiguous().reshape(1)
        grads = _lib.NodeHeadLossGrad(_ptr(g), None, _ptr(dl), None, None, None)
        with torch.cuda.device(lg.device):
            _lib.check(lib.node_head_loss_bwd(C.byref(_loss_struct(n, 0, o, ctx.reduction, target=target, logits=lg)), C.byref(grads),
                                              torch.cuda.current_stream(lg.device).cuda_stream))
        return dl, None, None


class _LinearCrossEntropy(torch.autograd.Function):
    """loss = CE(pooled @ W^T + b, target).  `logits` given: only the loss is computed forward (the Linear launch has
    happened: `linear`); None: Linear and loss in ONE forward launch.  Backward: ONE launch for d_pooled, d_weight, d_bias."""

    @staticmethod
    def forward(ctx, pooled, weight, bias, target, reduction, logits):
        lib = _lib.load()
        p, w = pooled.detach().contiguous(), weight.detach().contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        n, c = p.shape
        o = w.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        stat = torch.empty(2, dtype=torch.float32, device=p.device)
        with torch.cuda.device(p.device):
            scratch = _scratch(p.device, n)
            if logits is None:
                lg = torch.empty(n, o, dtype=torch.float32, device=p.device)
                h = _loss_struct(n, c, o, reduction, pooled=p, weight=w, bias=b, target=target, logits=lg, loss=loss,
                                 stat=stat, scratch=scratch)
            else:
                lg = logits.detach().contiguous()
                h = _loss_struct(n, 0, o, reduction, target=target, logits=lg, loss=loss, stat=stat, scratch=scratch)
            _lib.check(lib.node_head_loss_fwd(C.byref(h), torch.cuda.current_stream(p.device).cuda_stream))
        ctx.save_for_backward(p, w, lg, target)
        ctx.reduction, ctx.has_bias = reduction, bias is not None
        ctx.mark_non_differentiable(stat, lg)
        return loss, stat, lg

    @staticmethod
    def backward(ctx, g_loss, _g_stat, _g_logits):
        lib = _lib.load()
        p, w, lg, target = ctx.saved_tensors
        n, c = p.shape
        o = w.shape[0]
        dp, dw = torch.empty_like(p), torch.empty_like(w)
        db = torch.empty(o, dtype=torch.float32, device=p.device) if ctx.has_bias else None
        g = g_loss.contiguous().reshape(1)
        grads = _lib.NodeHeadLossGrad(_ptr(g), None, None, _ptr(dp), _ptr(dw), _ptr(db))
        with torch.cuda.device(p.device):
            h = _loss_struct(n, c, o, ctx.reduction, pooled=p, weight=w, target=target, logits=lg)
            _lib.check(lib.node_head_loss_bwd(C.byref(h), C.byref(grads), torch.cuda.current_stream(p.device).cuda_stream))
        return dp, dw, db, None, None, None


_REDUCTIONS = {'mean': _lib.REDUCE_MEAN, 'sum': _lib.REDUCE_SUM}


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, reduction: str = 'mean') -> torch.Tensor:
    """`F.cross_entropy(logits, target, reduction=...)` (train.py:43, :93) on the library's kernels: one launch forward,
    one backward; when `logits` came from `linear` (the classifier's last layer), that backward launch also produces
    the Linear layer's gradients.  The returned 0-d tensor carries `.node_stat` = device tensor {loss, correct
    predictions} for loops that read their running sums once per logging interval (train.py:44,46 read them per batch).
    CPU / non-fp32 / >1024-class inputs, class-probability targets and 'none' reduction go to PyTorch."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] <= 1024
            and target.is_cuda and target.dtype == torch.int64 and target.dim() == 1 and target.shape[0] == logits.shape[0]
            and reduction in _REDUCTIONS):
        return F.cross_entropy(logits, target, reduction=reduction)
    target = target.contiguous()
    src = getattr(logits, _LINEAR_ATTR, None) if torch.is_grad_enabled() else None
    if src is not None and (logits._version != src[3] or logits._backward_hooks or logits.retains_grad):
        src = None      # edited in place since `linear`, or somebody wants to see its gradient: the plain edge through `_Linear`
    if src is not None:
        # (the logits go in DETACHED: as an autograd input of the fused node they would pull `linear`'s own backward into the graph --
        #  called with a materialised zero gradient: a second, useless launch per step, seen in profiles/r05_cfg2_steps.txt's first cut)
        loss, stat, _ = _LinearCrossEntropy.apply(src[0], src[1], src[2], target, _REDUCTIONS[reduction], logits.detach())
    else:
        loss, stat = _CrossEntropy.apply(logits, target, _REDUCTIONS[reduction])
    loss.node_stat = stat
    return loss


def linear_cross_entropy(pooled, weight, bias, target, reduction: str = 'mean'):
    """(loss, logits) with Linear AND loss in one forward launch -- for loops that hand the targets to the model
    (`ODENet.loss`)."""
    if not (_fusable_linear(pooled, weight, bias) and target.is_cuda and target.dtype == torch.int64 and reduction in _REDUCTIONS):
        logits = F.linear(pooled, weight, bias)
        return F.cross_entropy(logits, target, reduction=reduction), logits
    loss, stat, logits = _LinearCrossEntropy.apply(pooled, weight, bias, target.contiguous(), _REDUCTIONS[reduction], None)
    loss.node_stat = stat
    return loss, logits


# ---------------------------------------------------------------------------------------------------------------
# The head of a whole trajectory [T, N, C, H, W] (the ODE block with `return_last_only = False`, model.py:39-40; the ResNet's
# taps, model.py:99) in one call.  Behind a GroupNorm there is nothing to add: the norm is per sample, `head_pool` / `gn_relu` /
# `linear` run one workgroup (one wave) per sample whatever the batch, and none of their launchers picks a kernel from n, so the
# T N samples of the flattened VIEW come out with the bits of T calls (`FCClassifier.forward`).  BatchNorm's statistics are per
# slice (the reference sends the slices through the norm one by one): `bn_head_pool_slices`.  The loss of the accuracy sweep
# (evaluate.py:258-262) and the trajectory distance of `attack diff` (diff.py:111-123) are one launch each.
# ---------------------------------------------------------------------------------------------------------------
_SLICES_SCRATCH = {}


def bn_head_slices_fusable(x: torch.Tensor, norm) -> bool:
    """What `bn_head_pool_slices` takes: a contiguous trajectory [T, N, C, H, W] whose slices `bn_head_fusable` accepts, outside
    autograd (the sliced entry is forward only)."""
    return (torch.is_tensor(x) and x.dim() == 5 and 1 <= x.shape[0] <= 65535 and x.is_contiguous() and bn_head_fusable(x[0], norm)
            and not (torch.is_grad_enabled() and (x.requires_grad or norm.weight.requires_grad or norm.bias.requires_grad)))


def bn_head_pool_slices(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """pooled[t, n, c] = mean_px relu(BatchNorm(x[t])), batch statistics of every slice its own: `bn_head_pool(x[t])` for all t
    in two launches (node_bnhead_fwd_slices), every slice the bits of its own call.  Forward only."""
    lib = _lib.load()
    T, n, c, h, w = x.shape
    shape = _lib.NodeBnfuncShape(n, c, h, w, eps)
    g, b = gamma.detach().contiguous(), beta.detach().contiguous()
    with torch.cuda.device(x.device):
        nbytes = lib.node_bnhead_slices_scratch_bytes(shape, T)
        if nbytes == 0:
            _lib.unsupported()
        pooled = torch.empty(T, n, c, device=x.device, dtype=torch.float32)
        stats = torch.empty(T, 2, c, device=x.device, dtype=torch.float32)
        scratch = torch.empty(nbytes // 8, device=x.device, dtype=torch.float64)
        _lib.check(lib.node_bnhead_fwd_slices(shape, T, _ptr(x), _ptr(g), _ptr(b), _ptr(pooled), _ptr(stats), _ptr(scratch),
                                              torch.cuda.current_stream(x.device).cuda_stream))
    return pooled


def _slices_scratch(device, slices, n):
    """Arrival counters + partials of the sliced loss: zero before the first use, left at zero by every launch; the counters'
    extent depends on `slices`, so one buffer per (device, stream, slices)."""
    lib = _lib.load()
    need = lib.node_head_loss_slices_scratch_bytes(int(slices), int(n)) // 4
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, int(slices))
    buf = _SLICES_SCRATCH.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.zeros(max(need, 1024), dtype=torch.float32, device=device)
        _SLICES_SCRATCH[key] = buf
    return buf


def trajectory_loss(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """[T, 2] = (summed cross-entropy, number of arg-max hits) of every slice of `logits` [T, N, classes] against the shared
    `target` [N] (int64): what the accuracy sweep accumulates per batch (evaluate.py:258-262).  fp32 logits on a HIP device with
    at most 1024 classes: ONE launch (node_head_loss_slices_fwd), every row the bits of `cross_entropy(logits[t], target,
    reduction='sum')` and its `.node_stat`; anything else: the same quantities through PyTorch.  No gradient."""
    if logits.dim() != 3 or target.dim() != 1 or target.shape[0] != logits.shape[1]:
        raise ValueError('trajectory_loss: logits [T, N, classes] and target [N], got %s and %s' % (tuple(logits.shape), tuple(target.shape)))
    T, n, o = logits.shape
    if not (logits.is_cuda and logits.dtype == torch.float32 and 1 <= o <= 1024 and 1 <= T <= 65535 and n >= 1
            and target.is_cuda and target.dtype == torch.int64):
        with torch.no_grad():
            loss = F.cross_entropy(logits.reshape(T * n, o), target.repeat(T), reduction='none').reshape(T, n).sum(1)
            hits = (logits.argmax(-1) == target.unsqueeze(0)).sum(-1)
            return torch.stack([loss, hits.to(loss.dtype)], 1)
    lib = _lib.load()
    lg, tg = logits.detach().contiguous(), target.contiguous()
    stat = torch.empty(T, 2, dtype=torch.float32, device=lg.device)
    with torch.cuda.device(lg.device):
        h = _lib.NodeHeadLossSlices(T, n, 0, o, None, None, None, _ptr(tg), _ptr(lg), None, _ptr(stat),
                                    _ptr(_slices_scratch(lg.device, T, n)))
        _lib.check(lib.node_head_loss_slices_fwd(C.byref(h), torch.cuda.current_stream(lg.device).cuda_stream))
    return stat


def _distance_fusable(traj0, traj1, norm):
    return (isinstance(norm, torch.nn.GroupNorm) and norm.affine and not norm._forward_hooks and not norm._forward_pre_hooks
            and traj0.is_cuda and traj0.dtype == torch.float32 and traj1.dtype == torch.float32 and traj1.device == traj0.device
            and traj0.shape[2] == norm.num_channels and traj0.numel() > 0
            and all(p.is_cuda and p.dtype == torch.float32 and p.device == traj0.device for p in (norm.weight, norm.bias)))


def trajectory_distance(traj0: torch.Tensor, traj1: torch.Tensor, norm):
    """(l2, cos), each [T, N]: Euclidean distance and cosine similarity of `relu(norm(.))` of two raw solver trajectories
    [T, N, C, H, W], flattened per (slice, sample) -- the two numbers per time point of adversarial/diff.py:111-123.  fp32
    trajectories on a HIP device behind an affine `nn.GroupNorm`: ONE launch that reads each trajectory once and writes
    neither normalised tensor (node_gn_relu_distance); anything else: the module chain of `diff.py`, slice by slice."""
    if traj0.dim() != 5 or traj0.shape != traj1.shape:
        raise ValueError('trajectory_distance: two trajectories [T, N, C, H, W] of one shape, got %s and %s'
                         % (tuple(traj0.shape), tuple(traj1.shape)))
    T, n, c, h, w = traj0.shape
    if not _distance_fusable(traj0, traj1, norm):
        with torch.no_grad():
            u0 = torch.stack([F.relu(norm(v)) for v in traj0]).reshape(T, n, -1)
            u1 = torch.stack([F.relu(norm(v)) for v in traj1]).reshape(T, n, -1)
            return (u1 - u0).pow(2).sum(-1).sqrt(), F.cosine_similarity(u1, u0, dim=-1)
    lib = _lib.load()
    a, b = traj0.detach().contiguous(), traj1.detach().contiguous()
    g, bt = norm.weight.detach().contiguous(), norm.bias.detach().contiguous()
    out = torch.empty(T, n, 2, dtype=torch.float32, device=a.device)
    shape = _lib.NodeShape(T * n, c, h, w, norm.num_groups, norm.eps)
    with torch.cuda.device(a.device):
        _lib.check(lib.node_gn_relu_distance(shape, _ptr(a), _ptr(b), _ptr(g), _ptr(bt), _ptr(out),
                                             torch.cuda.current_stream(a.device).cuda_stream))
    return out[..., 0], out[..., 1]

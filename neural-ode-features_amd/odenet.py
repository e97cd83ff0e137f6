"""The caller of the hot path: `ODENet` = stem -> ODEBlock -> classifier head.

Mirrors the observable semantics and state_dict keys of the reference's
`ODENet.forward` (`/root/reference/model.py:6-62`), its stems (`model.py:119-178`)
and head (`model.py:231-250`) so checkpoints load unchanged (`utils.py:248-270`).
The stem is a handful of plain convolutions run once per batch (~1 ODEfunc-eval of
FLOPs); the head's GroupNorm -> ReLU -> pool -> Dropout
is one fused HIP launch each way (head.py).  The stems that embed a second ODE block
(`ODEDownsample`, `ODEDownsample2`, model.py:181-223) run that block through the same
HIP solver; `StackedODENet` chains several blocks behind one stem (BASELINE.json
configs[4], a synthetic extension -- the reference stacks at most two).
"""
from __future__ import annotations

import torch
from torch import nn

from .imgconv import ImageConv2d
from .modules import ODEBlock, normalization


class ResBlock(nn.Module):
    """Pre-activation residual block (model.py:284-310)."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, norm='group'):
        super().__init__()
        make_norm = normalization(norm)
        self.norm1 = make_norm(inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.norm2 = make_norm(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)

    def forward(self, x):
        from .head import gn_relu   # fused GroupNorm + ReLU (one HIP launch each way) for CUDA fp32 inputs
        pre = gn_relu(x, self.norm1)
        skip = x if self.downsample is None else self.downsample(pre)
        h = self.conv2(gn_relu(self.conv1(pre), self.norm2))
        return h + skip


def _stem(kind, in_ch, out_ch, norm):
    """Stem bodies keyed like the reference's `--downsample` choices."""
    if kind == 'residual':       # model.py:167-178; forward / backward through the HIP library on a HIP device (stem.py)
        from .stem import ResidualStem
        return ResidualStem(
            nn.Conv2d(in_ch, 64, 3, 1),
            ResBlock(64, 64, stride=2, downsample=nn.Conv2d(64, 64, 1, 2, bias=False), norm=norm),
            ResBlock(64, out_ch, stride=2, downsample=nn.Conv2d(64, out_ch, 1, 2, bias=False), norm=norm))
    if kind == 'one-shot':       # model.py:119-126; forward / backward through the HIP library on a HIP device (imgconv.py)
        return ImageConv2d(in_ch, out_ch, 4, 2, 1)
    if kind in ('convolution', 'minimal'):   # model.py:129-164
        mid = 64 if kind == 'convolution' else 24
        make_norm = normalization(norm)
        from .convstem import ConvStem
        from .ministem import MinimalStem
        # forward / backward through the HIP library on a HIP device: the stem family's 64-column tiles (convstem.py) and, for
        # the 24 channels that do not fit them, kernels of their own (ministem.py)
        body = ConvStem if kind == 'convolution' else MinimalStem
        return body(
            nn.Conv2d(in_ch, mid, 3, 1), make_norm(mid), nn.ReLU(inplace=True),
            nn.Conv2d(mid, mid, 4, 2, 1), make_norm(mid), nn.ReLU(inplace=True),
            nn.Conv2d(mid, out_ch, 4, 2, 1))
    raise NotImplementedError('downsample=%r' % (kind,))


class StemTrajectory(tuple):
    """(trajectory, continuation) of an ODE stem in feature-extraction mode; `means` [T, N, C]: the trajectory's plane means where
    the stem has computed them along with the continuation (None: the caller pools)."""
    means = None


class ODEDownsample(nn.Module):
    """conv 4x4/2 -> ODE block -> max-pool 4x4/2 (model.py:181-196).  With `return_last_only` off the block
    returns its whole trajectory and this stem returns (trajectory, pooled last state)."""

    def __init__(self, in_ch, out_ch=64, method='dopri5', adjoint=False, t1=1, tol=1e-3, norm='group'):
        super().__init__()
        self.conv1 = ImageConv2d(in_ch, out_ch, 4, 2, 1)
        self.odeblock = ODEBlock(n_filters=out_ch, adjoint=adjoint, t1=t1, tol=tol, method=method, norm=norm)
        self.maxpool = nn.MaxPool2d(4, 2, 1)       # the geometry, and the path of everything the library's kernels do not take

    # the max-pool as one node of the HIP library (pool.py), and in feature extraction with a pool-only head the trajectory's
    # plane means from the same launch; False: nn.MaxPool2d and the caller's means, as before that node existed (A/B runs, tests)
    fused_pool = True

    def _fused(self):
        m = self.maxpool
        return self.fused_pool and (m.kernel_size, m.stride, m.padding, m.dilation, m.ceil_mode, m.return_indices) == (4, 2, 1, 1, False, False)

    def forward(self, x, with_means=False):
        """with_means: the caller's head only pools (`ODENet.forward`), so a trajectory comes back with its plane means"""
        x = self.odeblock(self.conv1(x))
        if x.dim() > 4:
            if with_means and self._fused():
                from .pool import fusable, trajectory_pool
                if fusable(x) and not (torch.is_grad_enabled() and x.requires_grad):
                    means, last = trajectory_pool(x)        # one launch: [T, N, C] and the second solve's initial state
                    out = StemTrajectory((x, last))
                    out.means = means
                    return out
            return StemTrajectory((x, self._pool(x[-1])))
        return self._pool(x)

    def _pool(self, x):
        if not self._fused():
            return self.maxpool(x)
        from .pool import max_pool_4s2
        return max_pool_4s2(x)


class ODEDownsample2(nn.Module):
    """conv 4x4/2 -> ODE block -> GroupNorm -> ReLU -> conv 4x4/2 (model.py:199-223)."""

    def __init__(self, in_ch, out_ch=64, method='dopri5', adjoint=False, t1=1, tol=1e-3, norm='group'):
        super().__init__()
        self.conv1 = ImageConv2d(in_ch, out_ch, 4, 2, 1)
        self.odeblock = ODEBlock(n_filters=out_ch, adjoint=adjoint, t1=t1, tol=tol, method=method, norm=norm)
        self.norm = nn.Sequential(normalization(norm)(out_ch), nn.ReLU(inplace=True))
        self.conv2 = nn.Conv2d(out_ch, out_ch, 4, 2, 1)
        self.apply_conv = False

    # the hand-off `conv2(norm(x))` as one node of the HIP library (downconv.py: `gn_relu_conv`, or `bn_relu_conv` with norm='batch')
    # where its kernels take the shape; False: the norm + ReLU and nn.Conv2d, as before those nodes existed (A/B runs, tests)
    fused_handoff = True

    def _norm(self, x):
        from .head import gn_relu
        return gn_relu(x, self.norm[0])

    def _handoff(self, x):
        if not self.fused_handoff:
            return self.conv2(self._norm(x))
        from . import downconv
        if isinstance(self.norm[0], nn.BatchNorm2d):      # norm='batch': the node of csrc/bndownconv_api.hip
            return downconv.bn_relu_conv(x, self.norm[0], self.conv2)
        return downconv.gn_relu_conv(x, self.norm[0], self.conv2)

    def _batch_trajectory(self, x):
        """`conv2(norm(slice))` of every slice of a `norm='batch'` trajectory [T, N, C, H, W] on the library's node, or None where it
        does not take the slices.  BatchNorm's statistics are per slice (model.py:214-216 sends the slices through the norm one by
        one), so the T slices are not one batch of T N samples: without gradients ONE sliced call normalises every slice with its
        own statistics (every slice the bits of its own call); with a backward possible, T calls, and autograd sums the shared
        parameters' gradients."""
        from . import downconv
        bn, conv, T = self.norm[0], self.conv2, x.shape[0]
        flat = x.reshape(-1, *x.shape[2:])
        if downconv.bn_fusable(flat, bn, conv, T):
            y = downconv.bn_relu_conv(flat, bn, conv, T)
            return y.reshape(T, x.shape[1], *y.shape[1:])
        if all(downconv.bn_fusable(xi, bn, conv) for xi in x):
            return torch.stack([downconv.bn_relu_conv(xi, bn, conv) for xi in x])
        return None

    def forward(self, x):
        x = self.odeblock(self.conv1(x))
        if x.dim() > 4:
            if self.apply_conv and self.fused_handoff and isinstance(self.norm[0], nn.BatchNorm2d):
                y = self._batch_trajectory(x)
                if y is not None:
                    return y, y[-1]
            elif self.apply_conv and self.fused_handoff:
                from .downconv import fusable, gn_relu_conv
                flat = x.reshape(-1, *x.shape[2:])
                if fusable(flat, self.norm[0], self.conv2):
                    # GroupNorm is per sample, so the T time slices are one batch of T N samples: one call instead of T, and
                    # every slice the bits of its own call (anything the kernels refuse keeps the per-slice modules below)
                    y = gn_relu_conv(flat, self.norm[0], self.conv2)
                    y = y.reshape(x.shape[0], x.shape[1], *y.shape[1:])
                    return y, y[-1]
            last = x[-1]
            x = torch.stack([self._norm(xi) for xi in x])
            if self.apply_conv:
                x = torch.stack([self.conv2(xi) for xi in x])
                return x, x[-1]
            return x, (self._handoff(last) if self.fused_handoff else self.conv2(x[-1]))
        return self._handoff(x)


class _Wrapped(nn.Module):
    """Holds a body under the attribute name `module` (state_dict key parity)."""

    def __init__(self, body):
        super().__init__()
        self.module = body

    def forward(self, x):
        return self.module(x)


class Flatten(nn.Module):
    def forward(self, x):
        return x.flatten(1)


class FCClassifier(_Wrapped):
    """GN -> ReLU -> global average pool -> [Dropout] -> Linear (model.py:231-250)."""

    def __init__(self, in_ch=64, out=10, dropout=0, norm='group'):
        layers = [normalization(norm)(in_ch), nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d((1, 1))]
        if dropout:
            layers.append(nn.Dropout(dropout))
        layers += [Flatten(), nn.Linear(in_ch, out)]
        super().__init__(nn.Sequential(*layers))

    def forward(self, x):
        """CUDA fp32 inputs take the fused HIP head (head.py: one launch forward, one backward; two each behind a
        `norm='batch'` BatchNorm2d that `head.bn_head_fusable` accepts) for everything in front of the last
        layer; anything else -- CPU tensors, a body someone has edited beyond what
        `ODENet.to_features_extractor` does -- runs the plain module sequence.  A trajectory [T, N, C, H, W] comes back as
        [T, N, out] (or [T, N, C] without the classification layer), slice t what `forward(x[t])` returns."""
        if x.dim() == 5:
            return self._trajectory(x)
        body = list(self.module.children())
        fusable = (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and len(body) in (5, 6)
                   and isinstance(body[1], nn.ReLU)
                   and isinstance(body[2], nn.AdaptiveAvgPool2d) and isinstance(body[-2], Flatten)
                   and (len(body) == 5 or isinstance(body[3], nn.Dropout))
                   and ((isinstance(body[0], nn.GroupNorm) and body[0].affine) or self._batch_head(x, body[0])))
        if not fusable:
            return self.module(x)
        pooled = self.pooled(x)
        last = body[-1]
        if isinstance(last, nn.Linear):      # one launch (head.linear); `cross_entropy` on its result fuses the two backwards
            from .head import linear
            return linear(pooled, last.weight, last.bias)
        return last(pooled)                  # (feature extraction: the classification layer was replaced, model.py:53)

    # a `norm='batch'` head as two launches of the HIP library each way (head.bn_head_pool); False: the module sequence, as before
    # those kernels existed (A/B runs, tests).  GroupNorm heads do not read it.
    fused_batch = True

    def _batch_head(self, x, norm):
        from .head import bn_head_fusable
        return self.fused_batch and bn_head_fusable(x, norm)

    # a trajectory [T, N, C, H, W] through the head in ONE call (a GroupNorm head: the nodes of a batch on the flattened view, T N
    # samples; a BatchNorm head: the sliced entry, statistics per slice); False: one call per slice, as before (A/B runs, tests)
    fused_trajectory = True

    def _trajectory_fusable(self, x):
        """The whole trajectory in one call: a HIP fp32 trajectory through an unedited, unhooked body that draws no dropout mask
        (the loop draws one mask per slice: the RNG stream must not change), and for a BatchNorm head what the forward-only sliced
        entry takes.  Everything else keeps the loop over the slices."""
        from .head import bn_head_slices_fusable
        body = list(self.module.children())
        if not (self.fused_trajectory and x.is_cuda and x.dtype == torch.float32 and x.shape[0] >= 1 and len(body) in (5, 6)
                and isinstance(body[1], nn.ReLU) and isinstance(body[2], nn.AdaptiveAvgPool2d) and isinstance(body[-2], Flatten)
                and (len(body) == 5 or isinstance(body[3], nn.Dropout))
                and (isinstance(body[-1], nn.Linear) or (isinstance(body[-1], nn.Sequential) and len(body[-1]) == 0))):
            return False
        if any(m._forward_hooks or m._forward_pre_hooks for m in self.modules()):
            return False
        if self.training and len(body) == 6 and body[3].p > 0:
            return False
        if isinstance(body[0], nn.GroupNorm):
            return body[0].affine
        return self.fused_batch and bn_head_slices_fusable(x, body[0])

    def _trajectory(self, x):
        if not self._trajectory_fusable(x):
            return torch.stack([self.forward(xi) for xi in x])
        from .head import bn_head_pool_slices, linear
        T, N = x.shape[:2]
        norm, last = self.module[0], self.module[-1]
        if isinstance(norm, nn.BatchNorm2d):
            pooled = bn_head_pool_slices(x, norm.weight, norm.bias, norm.eps).reshape(T * N, -1)
        else:
            # GroupNorm is per sample and the head's kernels run one workgroup (the Linear layer: one wave) per sample, picked from
            # (C, H W, out) alone: the T N samples of the view have the bits of T calls, and autograd goes through the same nodes
            pooled = self.pooled(x.reshape(T * N, *x.shape[2:]))
        out = linear(pooled, last.weight, last.bias) if isinstance(last, nn.Linear) else pooled
        return out.reshape(T, N, -1)

    def pooled(self, x):
        """dropout(mean_px relu(norm(x))): everything in front of the Linear layer, one launch each way (GroupNorm) or two
        (BatchNorm: statistics across the batch)."""
        from .head import bn_head_pool, head_pool
        body = list(self.module.children())
        gn = body[0]
        drop = body[3] if len(body) == 6 else None
        p, training = drop.p if drop is not None else 0.0, self.training and drop is not None
        if isinstance(gn, nn.BatchNorm2d):
            return bn_head_pool(x, gn.weight, gn.bias, gn.eps, p=p, training=training)
        return head_pool(x, gn.weight, gn.bias, gn.num_groups, gn.eps, p=p, training=training)


def head_on_trajectory(head, x):
    """`torch.stack([head(xi) for xi in x])` for a trajectory x [T, N, C, H, W] (model.py:39-40, :99) with ONE call of the head
    where it takes one: an `FCClassifier` (its `forward` decides what runs), or what `to_features_extractor(keep_pool=False)`
    leaves of it, `nn.Sequential(GroupNorm, ReLU)`, as `head.gn_relu` on the flattened view (GroupNorm is per sample).  A head
    with hooks of its own is called slice by slice, so that they see what they saw."""
    hooked = head._forward_hooks or head._forward_pre_hooks
    if isinstance(head, FCClassifier) and not hooked:
        return head(x)
    if (FCClassifier.fused_trajectory and not hooked and isinstance(head, nn.Sequential) and len(head) == 2
            and isinstance(head[0], nn.GroupNorm) and head[0].affine and isinstance(head[1], nn.ReLU)
            and x.is_cuda and x.dtype == torch.float32
            and not any(m._forward_hooks or m._forward_pre_hooks for m in head)):
        from .head import gn_relu
        return gn_relu(x.reshape(-1, *x.shape[2:]), head[0]).reshape(x.shape)
    return torch.stack([head(xi) for xi in x])


class ODENet(nn.Module):
    def __init__(self, in_ch, out=10, n_filters=64, downsample='residual', method='dopri5', tol=1e-3,
                 adjoint=False, t1=1, dropout=0, norm='group'):
        super().__init__()
        if downsample == 'ode':          # model.py:18-21
            self.downsample = ODEDownsample(in_ch, out_ch=n_filters, adjoint=adjoint, t1=t1, tol=tol, method=method, norm=norm)
        elif downsample == 'ode2':
            self.downsample = ODEDownsample2(in_ch, out_ch=n_filters, adjoint=adjoint, t1=t1, tol=tol, method=method, norm=norm)
        else:
            self.downsample = _Wrapped(_stem(downsample, in_ch, n_filters, norm))
        self.odeblock = ODEBlock(n_filters=n_filters, tol=tol, adjoint=adjoint, t1=t1, method=method, norm=norm)
        self.classifier = FCClassifier(in_ch=n_filters, out=out, dropout=dropout, norm=norm)

    def forward(self, x):
        out = []
        if isinstance(self.downsample, ODEDownsample):
            # a head that only pools (classification layer removed, model.py:53) takes the trajectory's plane means from the stem
            head = getattr(self.classifier, 'module', None)
            x = self.downsample(x, with_means=head is not None and isinstance(head[-1], nn.Sequential))
        else:
            x = self.downsample(x)
        if isinstance(x, (tuple, list)):     # an ODE stem in feature-extraction mode: (trajectory, continuation)
            means = getattr(x, 'means', None)
            f, x = x
            if means is not None:            # the stem's pool launch has produced them (pool.trajectory_pool)
                f = means
            elif isinstance(self.classifier.module[-1], nn.Sequential):   # classification layer removed: pool only
                f = torch.stack([fi.mean(-1).mean(-1) for fi in f])
            else:
                f = head_on_trajectory(self.classifier, f)
            out.append(f)
        x = self.odeblock(x)
        if x.dim() > 4:   # [T, N, C, H, W]: the head of every time slice (model.py:39-40), in one call where the head takes one
            x = head_on_trajectory(self.classifier, x)
        else:
            x = self.classifier(x)
        if not out:
            return x
        out.append(x)
        return torch.cat(out)

    def to_features_extractor(self, keep_pool=True):
        """model.py:48-56: expose the trajectory and drop the classification layer."""
        if isinstance(self.downsample, (ODEDownsample, ODEDownsample2)):
            self.downsample.odeblock.return_last_only = False
        self.odeblock.return_last_only = False
        if keep_pool:
            self.classifier.module[-1] = nn.Sequential()
        else:
            self.classifier = nn.Sequential(*list(self.classifier.module.children())[:2])

    def nfe(self, reset=False):
        count = self.odeblock.nfe
        if reset:
            self.odeblock.nfe = 0
        return count


class StackedODENet(nn.Module):
    """Residual stem -> `n_blocks` ODE blocks in series -> classifier head: BASELINE.json configs[4]
    ("4x-widened ODE-ResNet, 3 stacked ODE blocks").  A synthetic extension of `ODENet` (model.py:6-62; the
    reference stacks at most two blocks, through `ODEDownsample`); every block is the reference's `ODEBlock`
    and runs as its own HIP solve, keys `odeblocks.<i>.odefunc...`."""

    def __init__(self, in_ch, out=10, n_filters=64, n_blocks=3, downsample='residual', method='dopri5', tol=1e-3,
                 adjoint=False, t1=1, dropout=0, norm='group'):
        super().__init__()
        self.downsample = _Wrapped(_stem(downsample, in_ch, n_filters, norm))
        self.odeblocks = nn.ModuleList([ODEBlock(n_filters=n_filters, tol=tol, adjoint=adjoint, t1=t1, method=method,
                                                 norm=norm) for _ in range(n_blocks)])
        self.classifier = FCClassifier(in_ch=n_filters, out=out, dropout=dropout, norm=norm)

    @property
    def odeblock(self):       # the last block: what `ODENet` users read statistics from
        return self.odeblocks[-1]

    def forward(self, x):
        x = self.downsample(x)
        for blk in self.odeblocks:
            x = blk(x)
        return self.classifier(x)

    def nfe(self, reset=False):
        count = sum(b.nfe for b in self.odeblocks)
        if reset:
            for b in self.odeblocks:
                b.nfe = 0
        return count

"""The hand-off between the two solves of the `ode` stem -- `ODEDownsample.maxpool`, `nn.MaxPool2d(4, 2, 1)` of
the reference's `model.py:181-196` -- and the plane means of the stem's trajectory in feature extraction (`model.py:36`), through
the HIP library (`node_pool_fwd / node_pool_bwd`, csrc/pool_api.hip on the kernels of csrc/kernels_pool.hip): one launch each
way, ATen's results bit for bit, no atomics.  `max_pool_4s2(x)` is ONE autograd node whose backward is a gather over a saved
`uint8` argmax; `trajectory_pool(traj)` returns the means of every slice and the pooled last slice from one launch.  CPU tensors,
non-fp32 inputs, a trajectory that requires grad and a stream that is being captured run `F.max_pool2d` and
`mean(-1).mean(-1)` -- on a HIP device with the library missing, the fused path raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib


def _out_side(s):
    return (s - 2) // 2 + 1


# These launches are a few microseconds of device time, so what the call costs is its host side: no device switch where the
# tensor's device is the current one, and the stream's handle without a `torch.cuda.Stream` object around it.
_SAME_DEVICE = contextlib.nullcontext()
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _on(dev):
    return _SAME_DEVICE if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def _stream(dev):
    return _raw_stream(dev.index) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream


def _fwd(x, shape5, want_argmax, want_means):
    """x: fp32 contiguous on a HIP device, read as shape5 = (T, N, C, H, W) -> (pooled of the last slice, argmax or None, means or None)"""
    lib = _lib.load()
    t, n, c, h, w = shape5
    dev = x.device
    with _on(dev):
        pooled = torch.empty((n, c, _out_side(h), _out_side(w)), dtype=torch.float32, device=dev)
        argmax = torch.empty(pooled.shape, dtype=torch.uint8, device=dev) if want_argmax else None
        means = torch.empty((t, n, c), dtype=torch.float32, device=dev) if want_means else None
        _lib.check(lib.node_pool_fwd(C.byref(_lib.NodePoolShape(t, n, c, h, w)), x.data_ptr(), pooled.data_ptr(),
                                     argmax.data_ptr() if want_argmax else None, means.data_ptr() if want_means else None, _stream(dev)))
    return pooled, argmax, means


class _MaxPool4s2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep):
        ctx.in_shape = tuple(x.shape)
        pooled, argmax, _ = _fwd(x, (1,) + ctx.in_shape, keep, False)
        if keep:
            ctx.save_for_backward(argmax)       # all the backward needs: no workspace is carried, a second backward just runs
        return pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        lib = _lib.load()
        argmax, = ctx.saved_tensors
        n, c, h, w = ctx.in_shape
        dev = argmax.device
        grad_y = grad_y.contiguous()
        if grad_y.dtype != torch.float32:
            grad_y = grad_y.float()
        with _on(dev):
            d_x = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)       # every element is written by the kernel
            _lib.check(lib.node_pool_bwd(C.byref(_lib.NodePoolShape(1, n, c, h, w)), grad_y.data_ptr(), argmax.data_ptr(),
                                         d_x.data_ptr(), _stream(dev)))
        return d_x, None


def fusable(x) -> bool:
    """What the library's kernels take (node_pool_fwd): an fp32 contiguous batch [N, C, H, W] or trajectory [T, N, C, H, W] on a
    HIP device with every extent >= 1, sides from 2 to 32768 -- and a stream that is not being captured."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (4, 5) and x.is_contiguous()):
        return False
    if min(x.shape[:-2]) < 1 or min(x.shape[-2:]) < 2 or max(x.shape[-2:]) > 32768 or x.numel() > 1 << 40:
        return False
    return not torch.cuda.is_current_stream_capturing()


def max_pool_4s2(x):
    """`F.max_pool2d(x, 4, 2, 1)` of a batch [N, C, H, W]: one autograd node on the library's kernels where `fusable`."""
    if x.dim() != 4 or not fusable(x):
        return F.max_pool2d(x, 4, 2, 1)
    return _MaxPool4s2Fn.apply(x, torch.is_grad_enabled() and x.requires_grad)      # (the argmax is kept when a backward may follow)


def trajectory_pool(traj):
    """(means [T, N, C], pooled last slice [N, C, OH, OW]) of a trajectory [T, N, C, H, W] -- what
    `torch.stack([f.mean(-1).mean(-1) for f in traj])` and `F.max_pool2d(traj[-1], 4, 2, 1)` return -- from one launch where
    `fusable` and no gradient is asked for (the kernels have no backward through the means)."""
    if traj.dim() != 5:
        raise ValueError('trajectory_pool takes a trajectory [T, N, C, H, W], got %s' % (tuple(traj.shape),))
    if not fusable(traj) or (torch.is_grad_enabled() and traj.requires_grad):
        return torch.stack([f.mean(-1).mean(-1) for f in traj]), F.max_pool2d(traj[-1], 4, 2, 1)
    pooled, _, means = _fwd(traj, tuple(traj.shape), False, True)
    return means, pooled

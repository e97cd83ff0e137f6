"""The optimizer step of the training loop as ONE HIP launch.

The reference trains with `torch.optim.SGD(model.parameters(), lr, momentum=0.9, weight_decay=wd)`
(`/root/reference/train.py:136`), stepped and zeroed once per iteration (`train.py:56-58`).  `FusedSGD` does
the same arithmetic for every parameter tensor in one `node_sgd_step` launch per parameter group
(csrc/kernels_optim.hip): a table of (parameter, gradient, momentum) device pointers travels in the kernel
arguments, so gradients are read where autograd -- or the data-parallel reducer's all-reduce bucket
(`dp.GradientReducer`) -- left them.

It IS a `torch.optim.Optimizer`: the reference's LR schedulers (`LambdaLR`, `ReduceLROnPlateau`,
`CosineAnnealingLR`, train.py:158-163) drive it through `param_groups`, and its `state_dict()` has
torch.optim.SGD's layout (`state[i]['momentum_buffer']`), so `optimizer.load_state_dict(ckpt['optim'])`
(train.py:147) resumes a checkpoint written by the reference, and the reverse.

`FusedAdam` is the same for the reference's other choice, `Adam(params, lr, weight_decay=wd)` (`train.py:138`): one
`node_adam_step` per parameter group, torch.optim.Adam's `param_groups` keys and state layout (`step`, `exp_avg`,
`exp_avg_sq`), with the step counters in device memory so that a step skipped on the device is not counted.

No CPU path: parameters must live on a HIP device and the step raises if libnode_hip.so is missing.
"""
from __future__ import annotations

import torch

from . import _lib


class _Fused(torch.optim.Optimizer):
    """What the fused optimizers share: one launch of the library per parameter group over the parameters that have a
    gradient, the gradient scale, and the device flag that predicates the update (deferred completion).  A subclass
    refuses the modes it does not implement (`_refuse`) and fills and launches its table (`_launch`)."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self.grad_scale = 1.0        # dp.GradientReducer(average=False) leaves a SUM: set 1/world here
        # device float (1 element) or None: the step leaves everything untouched when it holds a non-zero value --
        # the commit point of a training step whose solves ran with deferred completion (integrate.Deferred)
        self.skip_flag = None
        self.flags_to_reset = []     # device tensors zeroed behind the step (the per-step miss flags): a step that forgot
                                     # to reset them could otherwise skip every later update silently

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        name = type(self).__name__
        for group in self.param_groups:
            self._refuse(group)
            pairs = []
            dev = None
            for p in group['params']:
                g = p.grad
                if g is None:                 # torch.optim skips parameters without a gradient
                    continue
                if not p.is_cuda:
                    raise RuntimeError('%s has no CPU path: parameters must live on a HIP device' % name)
                if p.dtype != torch.float32 or g.dtype != torch.float32 or g.device != p.device:
                    raise TypeError('%s needs float32 parameters and gradients on one device' % name)
                if not p.is_contiguous():
                    raise RuntimeError('%s needs contiguous parameters' % name)
                dev = dev or p.device
                if p.device != dev:
                    raise RuntimeError('one parameter group must live on one device')
                if not g.is_contiguous():
                    g = g.contiguous()
                pairs.append((p, g))          # (holds a contiguous copy of the gradient until the launch is enqueued)
            if not pairs:
                continue
            with torch.cuda.device(dev):
                self._launch(lib, group, pairs, self.skip_flag.data_ptr() if self.skip_flag is not None else None,
                             torch.cuda.current_stream(dev).cuda_stream)
        for f in self.flags_to_reset:
            f.zero_()
        return loss

    def use_deferred(self, deferred, reducer=None):
        """Predicate the update on `deferred`'s miss flag (see integrate.Deferred).  Under data parallelism the flag
        travels in the reducer's last bucket, so that every rank skips an update any rank missed."""
        if reducer is not None and (reducer.world > 1 or getattr(reducer, 'always', False)):
            self.skip_flag = reducer.carry_flag(deferred.miss_flag)
        else:
            self.skip_flag = deferred.miss_flag
        self.flags_to_reset = [deferred.miss_flag]
        deferred.armed = True


class FusedSGD(_Fused):
    """`torch.optim.SGD(params, lr, momentum, weight_decay)` with dampening 0 and no Nesterov (train.py:136).

        opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
        loss.backward(); opt.step(); opt.zero_grad()
    """

    def __init__(self, params, lr: float, momentum: float = 0.0, weight_decay: float = 0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError('lr, momentum and weight_decay must be non-negative')
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0, nesterov=False,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)

    def _refuse(self, group):
        if group.get('nesterov') or group.get('dampening') or group.get('maximize'):
            raise ValueError('FusedSGD implements plain SGD with momentum and weight decay (train.py:136): nesterov, '
                             'dampening and maximize are not supported (got %r)'
                             % {k: group.get(k) for k in ('nesterov', 'dampening', 'maximize')})

    def _launch(self, lib, group, pairs, skip, stream):
        rows = []
        for p, g in pairs:
            st = self.state[p]
            buf = st.get('momentum_buffer')
            if group['momentum'] == 0:
                buf = None                # torch.optim.SGD keeps no buffer then: same state_dict, half the memory
            elif buf is None:             # torch's first step sets buf = grad: zero + one fused step does the same
                buf = st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            rows.append((p.data_ptr(), g.data_ptr(), buf.data_ptr() if buf is not None else None, p.numel()))
        table = (_lib.NodeSgdTensor * len(rows))(*[_lib.NodeSgdTensor(*r) for r in rows])
        _lib.check(lib.node_sgd_step(table, len(rows), float(group['lr']), float(group['momentum']),
                                     float(group['weight_decay']), float(self.grad_scale), skip, stream))


class FusedAdam(_Fused):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay)` with amsgrad off and coupled L2 weight decay (train.py:138).

        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        loss.backward(); opt.step(); opt.zero_grad()

    `state[p]['step']` is an fp32 scalar tensor on the parameter's device (what torch.optim.Adam keeps with
    `capturable=True`): the device advances it, and only for a step it commits.  A count that arrives as a Python number
    or on another device -- a loaded torch.optim.Adam state has a CPU tensor -- is moved there by the next step."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        if lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError('lr, eps and weight_decay must be non-negative')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError('betas must lie in [0, 1)')
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)

    def _refuse(self, group):
        if group.get('amsgrad') or group.get('maximize') or group.get('decoupled_weight_decay'):
            raise ValueError('FusedAdam implements plain Adam with coupled weight decay (train.py:138): amsgrad, maximize '
                             'and decoupled_weight_decay are not supported (got %r)'
                             % {k: group.get(k) for k in ('amsgrad', 'maximize', 'decoupled_weight_decay')})

    def _launch(self, lib, group, pairs, skip, stream):
        rows = []
        for p, g in pairs:
            st = self.state[p]
            if 'exp_avg' not in st:
                st['step'] = torch.zeros((), dtype=torch.float32, device=p.device)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            step = st['step']
            if not (torch.is_tensor(step) and step.device == p.device and step.dtype == torch.float32 and step.numel() == 1):
                step = st['step'] = torch.tensor(float(step), dtype=torch.float32, device=p.device)
            m, v = st['exp_avg'], st['exp_avg_sq']
            if not (m.is_contiguous() and v.is_contiguous() and m.dtype == v.dtype == torch.float32
                    and m.device == v.device == p.device):
                raise TypeError('FusedAdam needs contiguous float32 exp_avg / exp_avg_sq on the device of their parameter')
            rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), p.numel()))
        table = (_lib.NodeAdamTensor * len(rows))(*[_lib.NodeAdamTensor(*r) for r in rows])
        beta1, beta2 = group['betas']
        _lib.check(lib.node_adam_step(table, len(rows), float(group['lr']), float(beta1), float(beta2), float(group['eps']),
                                      float(group['weight_decay']), float(self.grad_scale), skip, stream))

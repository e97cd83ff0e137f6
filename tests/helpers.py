"""Shared helpers for the parity tests (tests/ may import oracle/)."""
import contextlib
import copy
import ctypes
import os

import torch
import torch.nn.functional as F

from oracle.dynamics import OracleODEfunc, PARAM_ORDER, odefunc_vjp as oracle_vjp


def make_func(C, seed=0, device='cpu', kink_free=False):
    """An ODEfunc (package class) with non-trivial parameters + an oracle twin on CPU.

    kink_free=True shifts the GroupNorm biases in front of the two ReLUs to +8, so every
    pre-activation is positive and the ReLU derivative has no discontinuity anywhere near the data.
    Gradient parity through a whole solve can then be asserted tightly: with ordinary parameters one
    or two of the ~10^6 pre-activations of a solve land within fp32 rounding (~1e-6) of zero, two
    correct fp32 implementations then disagree on that element's ReLU mask, and the gradient changes
    by O(1) around that pixel (measured: the oracle against either GPU kernel generation, 4 of 6 seeds
    at [2, 256, 8, 8]).  The mask logic itself is covered by the single-evaluation VJP tests."""
    import neural_ode_features_amd as nof
    torch.manual_seed(seed)
    f = nof.ODEfunc(C)
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for name, p in f.named_parameters():
            if 'norm' in name and name.endswith('weight'):
                p.copy_(1.0 + 0.25 * torch.randn(p.shape, generator=gen))
            elif 'norm' in name and name.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
                if kink_free and not name.startswith('norm3'):
                    p.add_(8.0)
    twin = OracleODEfunc(C)
    twin.load_state_dict(f.state_dict())
    return f.to(device), twin


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def robust_grad_err(a, b):
    """(relative L2 error, fraction of elements off by more than 1e-3 x max|b|) -- for gradients that
    went through ReLU kinks, where a max-norm comparison is ill-posed (see make_func)."""
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    l2 = float((a - b).norm() / (b.norm() + 1e-30))
    frac = float(((a - b).abs() > 1e-3 * b.abs().max()).double().mean())
    return l2, frac


class ProbedODEfunc(OracleODEfunc):
    """The oracle dynamics, additionally recording per SAMPLE the smallest |pre-activation| either ReLU saw over
    every evaluation made through it (forward solve, and the recomputed forwards of the adjoint solve).  A sample
    whose record stays above the fp32 disagreement of two correct implementations (~1e-6) cannot have had a ReLU
    mask flip: its gradient must agree tightly.  Same ops in the same order as `oracle.dynamics.odefunc_forward`."""

    def __init__(self, dim):
        super().__init__(dim)
        self.min_abs = None

    def _note(self, z):
        m = z.detach().abs().flatten(1).amin(dim=1)
        self.min_abs = m if self.min_abs is None or self.min_abs.shape != m.shape else torch.minimum(self.min_abs, m)

    def forward(self, t, x):
        import torch.nn.functional as F
        from oracle.dynamics import concat_conv2d, n_groups
        self.nfe += 1
        p = dict(self.named_parameters())
        g = n_groups(x.shape[1])
        z1 = F.group_norm(x, g, p['norm1.weight'], p['norm1.bias'], 1e-5)
        self._note(z1)
        out = concat_conv2d(t, F.relu(z1), p['conv1._layer.weight'], p['conv1._layer.bias'])
        z2 = F.group_norm(out, g, p['norm2.weight'], p['norm2.bias'], 1e-5)
        self._note(z2)
        out = concat_conv2d(t, F.relu(z2), p['conv2._layer.weight'], p['conv2._layer.bias'])
        return F.group_norm(out, g, p['norm3.weight'], p['norm3.bias'], 1e-5)


def per_sample_err(a, b):
    """max |a - b| of every sample, relative to the largest |b| of the whole tensor."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return (a - b).abs().flatten(1).amax(dim=1) / (b.abs().max() + 1e-30)


_F64_DEVICE = None


def _arbiter_device():
    """Where the fp64 ARBITER leg of the oracle runs.  The oracle is PyTorch code; its fp64 convolutions on the host are what
    made the full-size arbiter tests the slowest of the suite (211 s for one case).  Where PyTorch-ROCm can run an fp64
    conv2d / group_norm forward + backward on the device (its own library path: nothing of this package), the arbiter runs
    there -- the fp32 oracle leg, the reference-equivalent one, always stays on the CPU.  NODE_TEST_ARBITER=cpu forces the host."""
    global _F64_DEVICE
    if _F64_DEVICE is None:
        _F64_DEVICE = 'cpu'
        if os.environ.get('NODE_TEST_ARBITER', 'auto') != 'cpu':
            try:
                gen = torch.Generator().manual_seed(0)
                x = torch.randn(2, 8, 8, 8, generator=gen, dtype=torch.float64)
                w = torch.randn(8, 8, 3, 3, generator=gen, dtype=torch.float64)
                xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
                yg = F.group_norm(F.conv2d(xg, wg, padding=1), 4)
                yg.square().sum().backward()
                xc, wc = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
                yc = F.group_norm(F.conv2d(xc, wc, padding=1), 4)
                yc.square().sum().backward()
                if float((yg.detach().cpu() - yc.detach()).abs().max()) < 1e-12 and float((wg.grad.cpu() - wc.grad).abs().max()) < 1e-10:
                    _F64_DEVICE = 'cuda'
            except Exception as e:     # no fp64 convolution on this PyTorch-ROCm build: the arbiter stays on the host
                print('fp64 arbiter stays on the CPU:', type(e).__name__, e)
    return _F64_DEVICE


@contextlib.contextmanager
def tune_env(**kw):
    """NODE_TUNE_* (or any) environment settings for the calls inside; the library reads them per call."""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def kink_free_replay(shape, envs, tol=1e-3, seed=53, t_end=1.0):
    """Kink-free parameters (make_func(kink_free=True): no ReLU mask can flip, so max-norm comparisons are meaningful) under the
    fp64 ARBITER, modelled on test_gpu_round2._replay_triplet.  Three kinds of solve, all of odeint_adjoint with dopri5:
      1. a free-running HIP solve under envs[0], recording the accepted step sizes of both directions (record_dt);
      2. for every settings dict of `envs`, a HIP replay of those steps (forced_dts / forced_dts_bwd) under it and
         NODE_TUNE_W4_STATS=1;
      3. the oracle's replay of the same steps in fp64 on _arbiter_device().
    Returns (free, [replay per env], fp64).  Each is a dict: 'out' (the state at t_end), 'gy' (grad_y0), 'gp' (the ten parameter
    gradients by name, in the order of named_parameters()); the HIP ones also 'fwd' / 'bwd' (the solves' statistics), 'nfe' (what
    func.nfe advanced by) and 'pair' (node_w4_pair_stats after the backward solve)."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import _lib
    from oracle import torchdiffeq_restated as tdq
    N, C, H, W = shape
    f, twin = make_func(C, seed=seed, device='cuda', kink_free=True)
    gen = torch.Generator().manual_seed(seed + 1)
    y = torch.randn(N, C, H, W, generator=gen)
    wgt = torch.randn(2, N, C, H, W, generator=gen) / (C * H * W) ** 0.5
    t = torch.tensor([0.0, t_end])

    def hip(env, options):
        for p in f.parameters():
            p.grad = None
        nfe0 = f.nfe
        with tune_env(NODE_TUNE_W4_STATS='1', **env):
            yh = y.cuda().requires_grad_(True)
            out = nof.odeint_adjoint(f, yh, t.cuda(), rtol=tol, atol=tol, method='dopri5', options=options)
            (out * wgt.cuda()).sum().backward()
            st = (ctypes.c_int32 * 4)()
            _lib.check(_lib.load().node_w4_pair_stats(st))
        return dict(out=out[-1].detach().cpu(), gy=yh.grad.cpu(), gp={n: p.grad.cpu() for n, p in f.named_parameters()},
                    fwd=dict(f.last_forward_stats), bwd=dict(f.last_backward_stats), nfe=f.nfe - nfe0, pair=list(st))

    free = hip(envs[0], {'record_dt': 1024})
    fs, bs = free['fwd'], free['bwd']
    fd = [d for d, a in zip(fs['dts'], fs['accepts']) if a]
    bd = [d for d, a in zip(bs['dts'], bs['accepts']) if a]
    assert len(fd) == fs['accepted'] and len(bd) == bs['accepted']
    print(shape, tol, 'free-running HIP: forward', (fs['accepted'], fs['rejected']), 'backward', (bs['accepted'], bs['rejected']))
    opts = {'forced_dts': fd, 'forced_dts_bwd': bd}
    reps = [hip(env, dict(opts)) for env in envs]
    dev = _arbiter_device()
    tw = copy.deepcopy(twin).to(torch.float64).to(dev)
    yo = y.to(torch.float64).to(dev).requires_grad_(True)
    out_o = tdq.odeint_adjoint(tw, yo, t.to(torch.float64).to(dev), rtol=tol, atol=tol, method='dopri5', options=dict(opts))
    (out_o * wgt.to(torch.float64).to(dev)).sum().backward()
    f64 = dict(out=out_o[-1].detach().cpu(), gy=yo.grad.cpu(), gp={n: p.grad.cpu() for n, p in tw.named_parameters()})
    print('  (fp64 arbiter ran on %s)' % dev)
    return free, reps, f64

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


# ----------------------------------------------------------------------------------------------------------------------
# The parameter gradient block by block (tests/test_param_blocks_host.py, tests/test_gpu_param_grads.py).
#
# rel_err over the flat vector of all 18 C^2 + 26 C gradients is one max-norm divided by the largest of them; the ten tensors
# differ in scale (the time-channel taps and the first GroupNorm's bias are ~1e-2 of the largest under the kink-free set), so
# a bound of 5e-5 on the flat vector is a bound of half a percent on those.  The blocks below are each compared at their OWN scale.
# ----------------------------------------------------------------------------------------------------------------------
TAPS = [(kh, kw) for kh in range(3) for kw in range(3)]


def param_grad_blocks(flat_or_dict, C):
    """The named blocks of a parameter gradient: the six GroupNorm vectors, the two conv biases and, for each conv weight
    [C][1 + C][3][3], the time-channel block `w[:, 0]` ('convK.w_t', [C, 3, 3]) and the nine data-tap blocks `w[:, 1:, kh, kw]`
    ('convK.tap<kh><kw>', [C, C]).  Takes the flat vector in parameters() order (what odefunc_vjp returns) or a mapping keyed
    like PARAM_ORDER; returns an ordered dict of fp64 CPU tensors."""
    if isinstance(flat_or_dict, dict):
        parts = {k: flat_or_dict[k].detach().double().cpu() for k in PARAM_ORDER}
    else:
        flat = flat_or_dict.detach().double().cpu().reshape(-1)
        assert flat.numel() == 18 * C * C + 26 * C, (flat.numel(), C)
        parts, o = {}, 0
        for k in PARAM_ORDER:
            n = 9 * C * (C + 1) if k.endswith('_layer.weight') else C
            parts[k] = flat[o:o + n]
            o += n
    out = {}
    for k in PARAM_ORDER:
        if k.endswith('_layer.weight'):
            w = parts[k].reshape(C, C + 1, 3, 3)
            name = k.split('.')[0]
            out[name + '.w_t'] = w[:, 0]
            for kh, kw in TAPS:
                out['%s.tap%d%d' % (name, kh, kw)] = w[:, 1:, kh, kw]
        elif k.endswith('_layer.bias'):
            out[k.split('.')[0] + '.bias'] = parts[k].reshape(C)
        else:
            out[k] = parts[k].reshape(C)
    return out


def block_scales(ref64, scales=None):
    """The scale of every block: max |ref64| over the block, unless `scales` names another one (the conv biases and vjp_t, whose
    true values are cancelled sums: odefunc_vjp_ref64)."""
    out = {k: float(v.abs().max()) for k, v in ref64.items()}
    out.update(scales or {})
    return out


def block_errors(got, ref64, scales=None):
    """max |got - ref64| / scale(block) for every block of ref64 (mappings of name -> tensor, param_grad_blocks's plus any scalar
    the caller adds, such as 'vjp_t')."""
    sc = block_scales(ref64, scales)
    errs = {}
    for k, r in ref64.items():
        g = torch.as_tensor(got[k]).detach().double().cpu().reshape(r.shape)
        errs[k] = float((g - r).abs().max()) / (sc[k] + 1e-300)
    return errs


def odefunc_vjp_ref64(t, y, params, cot, eps=1e-5):
    """The fp64 reference of one VJP of the dynamics: `oracle.dynamics.odefunc_forward` restated op by op in float64 on the CPU
    (nothing of the package is involved), with the two conv outputs kept so that their cotangents can be read.  `t` is rounded
    to fp32 first (the number every fp32 implementation is given).  Returns dict(f, vy, vt, vp (flat, parameters() order),
    blocks (param_grad_blocks of vp plus 'vjp_t'), scales): `scales` holds the blocks whose true value is a cancelled sum --
      * the conv biases: max_co sum_{n,h,w} |dL/d(conv output)|.  With one channel per group the GroupNorm behind the conv removes
        the bias exactly and the true gradient is identically zero; every implementation's value is the rounding of that sum;
      * vjp_t = sum_layers sum_{co,tap} W[co,0,tap] dL/dW[co,0,tap] / t: the sum of the terms' magnitudes."""
    from oracle.dynamics import concat_conv2d, n_groups
    t32 = float(torch.tensor(float(t), dtype=torch.float32))
    tt = torch.tensor(t32, dtype=torch.float64, requires_grad=True)
    x = y.detach().double().cpu().clone().requires_grad_(True)
    p = {k: params[k].detach().double().cpu().clone().requires_grad_(True) for k in PARAM_ORDER}
    g = n_groups(x.shape[1])
    C = x.shape[1]
    a1 = F.relu(F.group_norm(x, g, p['norm1.weight'], p['norm1.bias'], eps))
    c1 = concat_conv2d(tt, a1, p['conv1._layer.weight'], p['conv1._layer.bias'])
    c1.retain_grad()
    a2 = F.relu(F.group_norm(c1, g, p['norm2.weight'], p['norm2.bias'], eps))
    c2 = concat_conv2d(tt, a2, p['conv2._layer.weight'], p['conv2._layer.bias'])
    c2.retain_grad()
    f = F.group_norm(c2, g, p['norm3.weight'], p['norm3.bias'], eps)
    f.backward(cot.detach().double().cpu())
    grads = {k: v.grad for k, v in p.items()}
    blocks = param_grad_blocks(grads, C)
    blocks['vjp_t'] = tt.grad.detach().reshape(1)
    scales = {'conv1.bias': float(c1.grad.abs().sum(dim=(0, 2, 3)).max()), 'conv2.bias': float(c2.grad.abs().sum(dim=(0, 2, 3)).max())}
    vt_terms = sum(float((p[k][:, 0].detach() * grads[k][:, 0]).abs().sum()) for k in ('conv1._layer.weight', 'conv2._layer.weight'))
    scales['vjp_t'] = vt_terms / abs(t32)
    return dict(f=f.detach(), vy=x.grad, vt=float(tt.grad), vp=torch.cat([grads[k].reshape(-1) for k in PARAM_ORDER]),
                blocks=blocks, scales=scales)


def vjp_block_errors(vp, vt, ref):
    """block_errors of a VJP's (flat parameter gradient, vjp_t) against odefunc_vjp_ref64's result."""
    C = ref['f'].shape[1]
    got = param_grad_blocks(vp, C)
    got['vjp_t'] = torch.as_tensor(float(vt), dtype=torch.float64).reshape(1)
    return block_errors(got, ref['blocks'], ref['scales'])


def block_table(title, errs, ref, bound):
    """The per-block table of one case as text: error relative to the block's scale, the scale, and the scale relative to the
    largest gradient of the flat vector."""
    sc = block_scales(ref['blocks'], ref['scales'])
    gmax = float(ref['vp'].abs().max())
    lines = ['%s  (block bound %.1e)' % (title, bound)]
    for k, e in errs.items():
        lines.append('  %-14s err %.2e  scale %.3e  scale/max|vp| %.2e%s' % (k, e, sc[k], sc[k] / gmax, '' if e <= bound else '  <-- MISS'))
    return '\n'.join(lines)


def emit_table(text):
    """Print a case's table; NODE_PARAM_GRAD_TABLES=<file> also appends it there (how profiles/param_grad_blocks.txt is made)."""
    print(text, flush=True)
    path = os.environ.get('NODE_PARAM_GRAD_TABLES')
    if path:
        with open(path, 'a') as fh:
            fh.write(text + '\n')


def assert_param_blocks(title, ref, vp, vt, bound):
    """Every block of (vp, vt) within `bound` of odefunc_vjp_ref64's result `ref`, relative to the block's own scale; prints the
    per-block table first."""
    errs = vjp_block_errors(vp, vt, ref)
    emit_table(block_table(title, errs, ref, bound))
    over = {k: e for k, e in errs.items() if not e <= bound}
    assert not over, (title, over)
    return errs


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


# ----------------------------------------------------------------------------------------------------------------------
# One dopri5 / rk4 step of the FLAT solver (csrc/api_flat.hip), restated element by element.
#
# What `k_lincomb`, `k_init_norms` + `k_init_controller`, `k_error_norm` + `k_step_controller`, `k_emit_flat`, `k_commit`,
# `k_flat_scalar`, `k_flat_time` and `k_set_scalar_state` compute, as plain numpy.  Inputs are fp32 arrays; `F` is the
# precision the arithmetic runs in: np.float64 is the REFERENCE of tests/test_gpu_step_control.py, np.float32 the same
# statement at the kernels' precision (it only serves to MEASURE how far correct fp32 arithmetic lies from fp64, see
# SC_DEV_* below).  The coefficients are the kernels': every tableau entry rounded to fp32 FIRST (step_control.h c_CSOL /
# c_CERR, node_internal.h DP_CMID_F, butcher.h make_comb `(float)coef`, api_flat.hip `(float)DP_ALPHA`), then widened.
# tests/test_step_control_host.py pins this restatement to oracle/torchdiffeq_restated.py in fp64.
# ----------------------------------------------------------------------------------------------------------------------
import numpy as np

from oracle import torchdiffeq_restated as _tdq


def _r32(seq):
    return np.array(seq, dtype=np.float64).astype(np.float32)


SC_ALPHA = _r32(_tdq.DP_ALPHA)
SC_BETA = [_r32(row) for row in _tdq.DP_BETA]
SC_CSOL = _r32(_tdq.DP_C_SOL)
SC_CERR = _r32(_tdq.DP_C_ERROR)
SC_CMID = _r32(_tdq.DP_C_MID)
SC_RK4_ROWS = [_r32([1 / 3]), _r32([-1 / 3, 1.0]), _r32([1.0, -1.0, 1.0])]
SC_RK4_ALPHA = _r32([1 / 3, 2 / 3, 1.0])
SC_RK4_B = _r32([1 / 8, 3 / 8, 3 / 8, 1 / 8])
SC_TINY_H = float(np.float32(1e-6))      # upstream's `torch.tensor(1e-6)` is an fp32 number; the kernels' 1e-6f
SC_F0, SC_PROBE = -1, -2                 # _lib.FLAT_F0 / FLAT_PROBE
SC_NONFINITE = -6                        # NODE_ERR_NONFINITE


def sc_lincomb(y, ks, coef, scale, F=np.float64):
    """y + scale * sum_j coef_j k_j as k_lincomb forms it: cf_j = scale * coef_j, s = sum cf_j k_j, y + s."""
    y = np.asarray(y).astype(F)
    s = np.zeros_like(y)
    for c, k in zip(coef, ks):
        if c != 0:
            s = s + (F(scale) * F(c)) * np.asarray(k).astype(F)
    return y + s


def sc_stage(y, ks, t, dt, tsign, stage, method='dopri5', h0=None, F=np.float64):
    """(stage state or None, stage time) of node_flat_stage: dopri5 stages 0..5, rk4 stages 1..3, SC_F0 (time only), SC_PROBE."""
    if stage == SC_F0:
        return None, F(tsign) * (F(t) + F(0) * F(dt))
    if stage == SC_PROBE:
        return sc_lincomb(y, ks[:1], [1.0], h0, F), F(tsign) * (F(t) + F(h0))
    if method == 'dopri5':
        row, alpha = SC_BETA[stage], SC_ALPHA[stage]
    else:
        row, alpha = SC_RK4_ROWS[stage - 1], SC_RK4_ALPHA[stage - 1]
    return sc_lincomb(y, ks, row, dt, F), F(tsign) * (F(t) + F(alpha) * F(dt))


def sc_rk4_finish(y, ks, dt, F=np.float64):
    return sc_lincomb(y, ks, SC_RK4_B, dt, F)


def sc_rk4_finish_scalar(v, sk, dt, F=np.float64):
    """k_set_scalar_state(which = 1): ts_cur + (k0 + 3 k1 + 3 k2 + k3) * (dt / 8)."""
    sk = [F(np.float32(x)) for x in sk]
    return F(np.float32(v)) + (sk[0] + F(3) * sk[1] + F(3) * sk[2] + sk[3]) * (F(dt) * F(0.125))


def _sc_mean(sq, F):
    return F(np.sum(sq, dtype=F)) / F(sq.size)


def sc_initial_step(ys, f0s, f1_of, rtol, atol, scalar=None, F=np.float64):
    """Hairer's initial step over 1..3 segments (+ the scalar segment: scalar = (value, f0), f1_of's second result its f1).
    `f1_of(h0)` -> (list of f1 per segment, scalar f1 or None): what the caller's dynamics return at the probe.
    Returns dict(h0, dt, d0, d1, d2) with d* the per-segment lists (scalar last)."""
    rtol, atol = F(np.float32(rtol)), F(np.float32(atol))
    ys = [np.asarray(y).astype(F) for y in ys]
    f0s = [np.asarray(f).astype(F) for f in f0s]
    scs = [atol + np.abs(y) * rtol for y in ys]
    d0 = [np.sqrt(_sc_mean((y / sc) ** 2, F)) for y, sc in zip(ys, scs)]
    d1 = [np.sqrt(_sc_mean((f / sc) ** 2, F)) for f, sc in zip(f0s, scs)]
    if scalar is not None:
        sv, sf0 = F(np.float32(scalar[0])), F(np.float32(scalar[1]))
        ssc = atol + abs(sv) * rtol
        d0.append(abs(sv / ssc))
        d1.append(abs(sf0 / ssc))
    with np.errstate(divide='ignore', invalid='ignore'):
        q = [a / b for a, b in zip(d0, d1)]
    d0m, d1m = max(d0), max(d1)
    if d0m < 1e-5 or d1m < 1e-5:
        h0 = F(SC_TINY_H)
    else:
        h0 = F(0.01) * F(np.fmax.reduce(np.array(q, dtype=F)))
    f1s, sf1 = f1_of(float(h0))
    d2 = [np.sqrt(_sc_mean(((np.asarray(f1).astype(F) - f0) / sc) ** 2, F)) / h0 for f1, f0, sc in zip(f1s, f0s, scs)]
    if scalar is not None:
        d2.append(abs((F(np.float32(sf1)) - sf0) / ssc) / h0)
    d2m = max(d2)
    if d1m <= 1e-15 and d2m <= 1e-15:
        h1 = max(F(SC_TINY_H), h0 * F(1e-3))
    else:
        h1 = (F(0.01) / max(d1m, d2m)) ** F(0.2)
    return dict(h0=float(h0), dt=float(min(F(100) * h0, h1)), d0=d0, d1=d1, d2=d2)


def sc_error_ratios(ys, y1s, ks, dt, rtol, atol, scalar=None, F=np.float64, cerr=None):
    """Mean squared error ratio of every segment (the scalar segment's last; scalar = (value, [k0..k6])).
    Returns (ratios, per-element squared ratios of the tensor segments, the scalar segment's end-of-step value or None)."""
    cerr = SC_CERR if cerr is None else cerr
    rtol, atol = F(np.float32(rtol)), F(np.float32(atol))
    ratios, elems = [], []
    for y, y1, k in zip(ys, y1s, ks):
        y, y1 = np.asarray(y).astype(F), np.asarray(y1).astype(F)
        e = np.zeros_like(y)
        for j in (0, 2, 3, 4, 5, 6):
            e = e + (F(dt) * F(cerr[j])) * np.asarray(k[j]).astype(F)
        r = e / (atol + rtol * np.maximum(np.abs(y), np.abs(y1)))
        elems.append(r * r)
        ratios.append(_sc_mean(r * r, F))
    s_new = None
    if scalar is not None:
        sv, sk = F(np.float32(scalar[0])), [F(np.float32(x)) for x in scalar[1]]
        e = s = F(0)
        for j in (0, 2, 3, 4, 5, 6):
            e = e + (F(dt) * F(cerr[j])) * sk[j]
            if j < 6:
                s = s + (F(dt) * F(SC_CSOL[j])) * sk[j]
        s_new = sv + s
        r = e / (atol + rtol * max(abs(sv), abs(s_new)))
        ratios.append(r * r)
    return ratios, elems, s_new


def sc_dt_next(dt, maxr):
    """`_optimal_step_size` on the largest ratio: (dt_next, regime) with regime 'x10' (ratio 0), 'clamp' ([0.1, 1 / dfactor]
    reached) or 'free'."""
    maxr = float(maxr)
    if maxr == 0.0:
        return dt * 10.0, 'x10'
    dfactor = 1.0 if maxr < 1.0 else 0.2
    # (upstream's exponent and lower clamp are fp32 numbers, `torch.tensor(1.0 / order)`; the kernel's pow(er, 0.2) differs from that by
    # |ln er| * 3e-9 relative, far inside the fp32 tolerance of the GPU tests)
    factor = (maxr ** 0.5) ** float(np.float32(0.2)) / 0.9
    clamped = min(max(factor, float(np.float32(0.1))), 1.0 / dfactor)
    return dt / clamped, ('free' if clamped == factor else 'clamp')


def sc_decide(ratios, t, dt, targets, j=0):
    """The step controller's decision from the segments' ratios: accept iff every ratio <= 1; t advances when accepted; the
    targets [j0, j1) passed (target <= t_new); done once every target is passed; a NaN or infinite ratio stops the solve."""
    rs = [float(r) for r in ratios]
    if any(not np.isfinite(r) for r in rs):
        return dict(accept=False, status=SC_NONFINITE, dt_next=dt, t=t, j0=j, j1=j, done=True, regime='nonfinite', maxr=float('nan'))
    accept = all(r <= 1.0 for r in rs)
    maxr = max(rs)
    dt_next, regime = sc_dt_next(dt, maxr)
    t_new, j1 = t, j
    if accept:
        t_new = t + dt
        while j1 < len(targets) and not (targets[j1] > t_new):
            j1 += 1
    return dict(accept=accept, status=0, dt_next=dt_next, t=t_new, j0=j, j1=j1, done=accept and j1 == len(targets),
                regime=regime, maxr=maxr)


def sc_dense(y0, y1, k, dt, t0, t1, target, F=np.float64, cmid=None):
    """The quartic of `_interp_fit_dopri5` + `_interp_evaluate` at `target` in [t0, t1], in interp_one's order of operations
    (arrays or scalars; k = the seven stage derivatives, k[1] has weight zero)."""
    cmid = SC_CMID if cmid is None else cmid
    conv = (lambda a: np.asarray(a).astype(F))
    y0, y1, k, dt = conv(y0), conv(y1), [conv(a) for a in k], F(dt)
    s = np.zeros_like(y0)
    for j in (0, 2, 3, 4, 5, 6):
        s = s + (dt * F(cmid[j])) * k[j]
    ymid, f0, f1 = y0 + s, k[0], k[6]
    x = (F(target) - F(t0)) / (F(t1) - F(t0))
    ca = (F(-2) * dt) * f0 + (F(2) * dt) * f1 + F(-8) * y0 + F(-8) * y1 + F(16) * ymid
    cb = (F(5) * dt) * f0 + (F(-3) * dt) * f1 + F(18) * y0 + F(14) * y1 + F(-32) * ymid
    cc = (F(-4) * dt) * f0 + dt * f1 + F(-11) * y0 + F(-5) * y1 + F(16) * ymid
    cd = dt * f0
    x2 = x * x
    x3 = x2 * x
    x4 = x3 * x
    return ca * x4 + cb * x3 + cc * x2 + cd * x + y0


def sc_finish_step(st, targets, j=0, F=np.float64):
    """One node_flat_finish_step(dopri5) on the state `st` (sc_case): the decision (sc_decide) plus 'ratios', 'rows' (dense
    output of segment 0 for every target passed, by row), 's_new' (the scalar segment at the end of the step) and, when the step
    ends an augmented solve, 'final' (every segment and the scalar at the last target)."""
    ratios, _, s_new = sc_error_ratios(st['y'], st['y1'], st['k'], st['dt'], st['rtol'], st['atol'], st['scalar'], F)
    d = sc_decide(ratios, st['t'], st['dt'], targets, j)
    d.update(ratios=ratios, s_new=s_new, rows={}, final=None)
    for jj in range(d['j0'], d['j1']):
        d['rows'][jj] = sc_dense(st['y'][0], st['y1'][0], st['k'][0], st['dt'], st['t'], d['t'], targets[jj], F)
    if d['done'] and d['status'] == 0 and st['scalar'] is not None and d['j1'] > d['j0']:
        segs = [sc_dense(y, y1, k, st['dt'], st['t'], d['t'], targets[-1], F) for y, y1, k in zip(st['y'], st['y1'], st['k'])]
        sk = [np.float32(x) for x in st['scalar'][1]]
        d['final'] = (segs, sc_dense(np.float32(st['scalar'][0]), s_new, sk, st['dt'], st['t'], d['t'], targets[-1], F))
    return d


def sc_case(numels, ratios, seed=0, has_scalar=False, spike=None, t=0.25, dt=0.0625, rtol=1e-3, atol=1e-4):
    """Seeded Gaussian buffers of a flat state whose segments have the mean squared error ratios `ratios` (one per tensor segment,
    then the scalar segment's): y, y1 = y + 0.1 N(0, 1), k[0..6] ~ N(0, 1) scaled per segment -- y1 is a buffer of its own to the
    kernels, so a segment's ratio is exactly quadratic in the scale of its k.  spike = (segment, index): that element carries
    three quarters of its segment's sum.  ratio 0: all-zero derivatives."""
    rng = np.random.default_rng(1000 + seed)
    f32 = np.float32
    ys = [rng.standard_normal(n).astype(f32) for n in numels]
    for y in ys:
        y[0] = 2.0        # (per-element tolerances are relative to max|y|: a segment of one or three elements must not make that tiny)
    y1s = [(y + 0.1 * rng.standard_normal(y.size)).astype(f32) for y in ys]
    ks = [[rng.standard_normal(n).astype(f32) for _ in range(7)] for n in numels]
    scalar = None
    if has_scalar:
        scalar = (f32(rng.standard_normal()), [f32(v) for v in rng.standard_normal(7)])
    if spike is not None:
        sg, idx = spike
        _, elems, _ = sc_error_ratios(ys, y1s, ks, dt, rtol, atol)
        rr = elems[sg]
        want = 3.0 * (rr.sum() - rr[idx])
        tol_i = atol + rtol * max(abs(float(ys[sg][idx])), abs(float(y1s[sg][idx])))
        e_i = np.sqrt(rr[idx]) * tol_i
        ks[sg][6][idx] = f32(ks[sg][6][idx] + (np.sqrt(want) * tol_i + e_i) / (dt * abs(float(SC_CERR[6]))))
    for _ in range(30):
        got, _, _ = sc_error_ratios(ys, y1s, ks, dt, rtol, atol, scalar)
        for i, (g, w) in enumerate(zip(got, ratios)):
            sc = 0.0 if w == 0 else float(np.sqrt(w / g))
            if i < len(numels):
                ks[i] = [(k.astype(np.float64) * sc).astype(f32) for k in ks[i]]
            else:
                scalar = (scalar[0], [f32(float(v) * sc) for v in scalar[1]])
        if all(w == 0 or abs(g / w - 1) < 1e-3 for g, w in zip(got, ratios)):
            break
    return dict(y=ys, y1=y1s, k=ks, scalar=scalar, t=t, dt=dt, rtol=rtol, atol=atol, numels=list(numels))


# The sizes at which the kernels' indexing changes (derivation: tests/test_gpu_step_control.py)
SC_SMALL = [1, 3, 4, 5, 255, 1027]
SC_N_INIT = 131072 + 1
SC_N_ERR = 524288 + 5
SC_N_COMMIT = 2097152 + 5

# (name, sc_case arguments, band): band 'free' = accepted, dt_next unclamped (largest ratio in [0.01, 0.3]); 'clamp' = accepted,
# dt_next == dt (ratio in [0.45, 0.85]); 'reject' = rejected, unclamped ([2, 1e4]); 'huge' = rejected, dt / 5; 'zero' = dt x 10
SC_STEP_CASES = (
    [('n%d' % n, dict(numels=[n], ratios=[0.1], seed=n), 'free') for n in SC_SMALL] +
    [('sweep2', dict(numels=[SC_N_ERR], ratios=[0.2], seed=7), 'free'),
     ('commit2', dict(numels=[SC_N_COMMIT], ratios=[0.15], seed=8), 'free')] +
    [('spike1027_%d' % i, dict(numels=[1027], ratios=[0.1 if i % 2 == 0 else 50.0], seed=20 + i, spike=(0, i)),
      'free' if i % 2 == 0 else 'reject') for i in (0, 1020, 1023, 1024, 1025, 1026)] +
    [('spikebig_%d' % i, dict(numels=[SC_N_ERR], ratios=[0.1], seed=30, spike=(0, i)), 'free')
     for i in (0, SC_N_ERR - 5, SC_N_ERR - 2, SC_N_ERR - 1)] +
    [('seg3_last_rejects', dict(numels=[SC_N_ERR, 7, 1], ratios=[0.2, 0.2, 50.0], seed=40), 'reject'),
     ('seg3_middle_max', dict(numels=[SC_N_ERR, 7, 1], ratios=[0.05, 0.2, 0.1], seed=41), 'free'),
     ('seg2', dict(numels=[5, 1027], ratios=[0.05, 0.2], seed=42), 'free'),
     ('seg2_scalar_rejects', dict(numels=[5, 1027], ratios=[0.2, 0.2, 5.0], seed=43, has_scalar=True), 'reject'),
     ('seg2_scalar', dict(numels=[5, 1027], ratios=[0.1, 0.05, 0.2], seed=44, has_scalar=True), 'free'),
     ('seg3_scalar', dict(numels=[SC_N_ERR, 7, 1], ratios=[0.1, 0.05, 0.2, 0.1], seed=46, has_scalar=True), 'free'),
     ('seg2_scalar_small', dict(numels=[5, 1027], ratios=[0.2, 0.1, 0.05], seed=45, has_scalar=True), 'free'),
     ('clamp', dict(numels=[1027], ratios=[0.65], seed=50), 'clamp'),
     ('huge', dict(numels=[255], ratios=[1e9], seed=51), 'huge'),
     ('zero', dict(numels=[1027], ratios=[0.0], seed=52), 'zero')])
SC_BANDS = {'free': (0.01, 0.3), 'clamp': (0.45, 0.85), 'reject': (2.0, 1e4), 'huge': (4.5 ** 10 * 1.1, float('inf')), 'zero': (0.0, 0.0)}


def sc_init_case(name):
    """Inputs of the initial-step cases: dict(y, f0, f1 (lists per segment), scalar = (value, f0, f1) or None)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    f32 = np.float32
    g = (lambda n, s=1.0: (s * rng.standard_normal(n)).astype(f32))
    scalar = None
    if name.startswith('n'):                       # ordinary, one segment of the given size
        n = int(name[1:])
        y, f0 = [g(n)], [g(n)]
        f1 = [(f0[0] + g(n, 0.01)).astype(f32)]
    elif name == 'y_zero':                         # d0 < 1e-5: h0 = 1e-6
        y, f0 = [np.zeros(1027, f32)], [g(1027)]
        f1 = [(f0[0] + g(1027, 1e-4)).astype(f32)]
    elif name == 'f_zero':                         # d1, d2 <= 1e-15
        y, f0, f1 = [g(1027)], [np.zeros(1027, f32)], [np.zeros(1027, f32)]
    elif name == 'seg3':                           # segment 0: max d0 / d1; segment 1: max d1; segment 2: max d2
        y = [g(SC_N_INIT, 4.0), g(7), g(1)]
        f0 = [g(SC_N_INIT, 0.5), g(7, 8.0), g(1)]
        f1 = [(f0[0] + g(SC_N_INIT, 1e-3)).astype(f32), (f0[1] + g(7, 1e-3)).astype(f32), (f0[2] + f32(0.5)).astype(f32)]
    elif name == 'scalar_max':                     # the scalar segment supplies every maximum
        y, f0 = [g(5, 1e-3), g(1027, 1e-3)], [g(5, 1e-3), g(1027, 1e-3)]
        f1 = [(a + g(a.size, 1e-6)).astype(f32) for a in f0]
        scalar = (f32(40.0), f32(20.0), f32(29.0))
    elif name == 'seg2_scalar':                    # scalar present, maxima from the tensors
        y, f0 = [g(5), g(1027)], [g(5), g(1027)]
        f1 = [(a + g(a.size, 1e-2)).astype(f32) for a in f0]
        scalar = (f32(0.005), f32(0.02), f32(0.02 + 1e-6))
    else:
        raise KeyError(name)
    return dict(y=y, f0=f0, f1=f1, scalar=scalar)


SC_INIT_CASES = ['n%d' % n for n in SC_SMALL + [SC_N_INIT]] + ['y_zero', 'f_zero', 'seg3', 'scalar_max', 'seg2_scalar']
SC_INIT_TOL = (1e-3, 1e-4)                        # rtol, atol of the initial-step cases

# Largest relative deviation of the SAME restatement run in fp32 on the CPU from its fp64 run, over the cases above (measured by
# tests/test_step_control_host.py, which asserts that they still hold): what correct fp32 arithmetic costs.  The kernels sum in
# another order, so they get 8 x these (tests/test_gpu_step_control.py); nothing here comes from a kernel's output.
SC_DEV_RATIO = 5e-7  # measured 4.6e-7:   # mean squared error ratio of a segment
SC_DEV_INIT = 1.6e-7  # measured 1.53e-7:    # h0 and the initial dt
SC_DEV_STAGE = 6e-8  # measured 5.9e-8:   # a stage state / RK4 update per element, relative to max|y|; a stage time, relative
SC_DEV_DENSE = 4.2e-6  # measured 4.13e-6:   # dense output per element, relative to max|y|


def sc_advance(st, d, dt_next):
    """The state after an accepted step that did not end the solve (k_commit + the controller's scalar bookkeeping): y <- y1,
    k0 <- k6 (FSAL), the scalar segment likewise; t and dt move on.  Every other buffer is the caller's and stays."""
    new = dict(st)
    new['y'] = [a.copy() for a in st['y1']]
    new['k'] = [[k[6].copy()] + [a.copy() for a in k[1:]] for k in st['k']]
    if st['scalar'] is not None:
        sk = list(st['scalar'][1])
        new['scalar'] = (np.float32(d['s_new']), [sk[6]] + sk[1:])
    new['t'], new['dt'] = d['t'], dt_next
    return new


SC_DENSE_SIZES = [5, 1027, SC_N_ERR]


def sc_dense_scenario(n):
    """Three consecutive steps on one state: the first passes THREE targets (the last one exactly t + dt), the second ONE, the
    third NONE.  Returns (state, targets)."""
    st = sc_case([n], [0.05], seed=60 + n % 97)
    dt2, _ = sc_dt_next(st['dt'], 0.05)
    t, dt = st['t'], st['dt']
    return st, [t + 0.3 * dt, t + 0.5 * dt, t + dt, t + dt + 0.5 * dt2, t + 10.0]


# ----------------------------------------------------------------------------------------------------------------------
# The adjoint's time gradients (tests/test_gpu_adjoint_time.py, tools/adjoint_time_d32.py).
#
# node_solve_adjoint's third output, grad_t [n_t], in upstream's `time_vjps` order: grad_t[0] is the integrated adj_time,
# grad_t[i] = <f(t_i, y_i), dL/dy_i> for i >= 1.  The reference is the oracle's `odeint_adjoint` with a time grid that requires
# grad.  A case = (shape, grid, method, mode); mode 'replay' forces the step sizes below in both directions (both sides repeat
# a list's last entry until the interval's end is passed and restart the backward list at every interval, so one list serves
# any grid and no step lands on a target: every interval ends in dense output), 'free' lets the controller run, rk4 has no
# step sizes to force.
# ----------------------------------------------------------------------------------------------------------------------
AT_FWD_DTS = [0.07, 0.11, 0.13]
AT_BWD_DTS = [0.06, 0.09, 0.14]
AT_ALIGN = (1.0, -0.7, 0.5, 0.8)      # c_i: how much of f(t_i, y_i)'s direction slice i of the cotangent carries
AT_TOL = 1e-3
AT_SEED = 61

# family -> (shape, what node_describe_dims must say of it): the smallest shape of each kernel family an adjoint solve can take
AT_FAMILIES = {
    'small-C': ((2, 16, 4, 4), dict(wino4=0, wgrad_kernel='W2_4', conv_kernel='W1_64')),      # C below one channel tile, units of 4 tiles
    'fp32': ((3, 32, 8, 8), dict(wino4=0, wgrad_kernel='W2_8', conv_kernel='W1_64')),         # fp32 convolution + fp32 weight gradient
    'w4-8x8': ((8, 64, 8, 8), dict(wino4=1, w4q=1)),                                          # F(4x4,3x3) pipeline, 8 x 8 states
    'w4-16x16': ((2, 128, 16, 16), dict(wino4=1, w4q=4)),                                     # ... its 16 x 16 quadrant passes
}
AT_GRIDS = [(0.0, 0.3, 0.55, 1.0), (1.0, 0.4, 0.0), (1.0, 0.25), (0.0, 1.0)]
# (family, grid, method, mode) of every comparison with the oracle
AT_DOPRI5 = ([(fam, g, 'dopri5', 'replay') for fam in ('small-C', 'fp32') for g in AT_GRIDS] +
             [(fam, g, 'dopri5', 'replay') for fam in ('w4-8x8', 'w4-16x16') for g in AT_GRIDS[:2]])
AT_RK4 = [(fam, g, 'rk4', 'fixed') for fam in ('small-C', 'fp32') for g in AT_GRIDS[:2]]


# bound on the grad_t error of (method, family): 8 x the family's largest d32 (the fp32 CPU oracle's own distance from the fp64
# arbiter, tools/adjoint_time_d32.py -> profiles/adjoint_time_grads.txt), rounded up to one significant digit
AT_GT_TOL = {('dopri5', 'small-C'): 7e-6, ('dopri5', 'fp32'): 8e-6, ('dopri5', 'w4-8x8'): 2e-5, ('dopri5', 'w4-16x16'): 4e-6,
             ('rk4', 'small-C'): 7e-7, ('rk4', 'fp32'): 2e-6}
# every grad_t entry is at least this fraction of sum_j ||f_j|| ||g_j|| under the aligned cotangent (measured 0.050 ... 0.27 over the
# cases; a random cotangent gives ~1e-3): below it the relative bound above would be a bound on a cancelled sum
AT_MIN_COND = 0.04


def at_id(fam, grid, method, mode):
    return '%s-%s-%s-%s' % (fam, 'x'.join('%d' % d for d in AT_FAMILIES[fam][0]), method, '_'.join('%g' % v for v in grid))


_AT_CASES = {}


def at_options(method, mode):
    return {'forced_dts': list(AT_FWD_DTS), 'forced_dts_bwd': list(AT_BWD_DTS)} if (method == 'dopri5' and mode == 'replay') else None


def _at_oracle(twin, y, t, g, method, options):
    """The oracle's adjoint solve with t.requires_grad: dict(out, gy, gp (flat, parameters() order), gt, fwd, bwd)."""
    from oracle import torchdiffeq_restated as tdq
    for p in twin.parameters():
        p.grad = None
    yo = y.clone().requires_grad_(True)
    to = t.clone().requires_grad_(True)
    fs, bs = tdq.SolverStats(), tdq.SolverStats()
    out = tdq.odeint_adjoint(twin, yo, to, rtol=AT_TOL, atol=AT_TOL, method=method, options=dict(options) if options else None,
                             fwd_stats=fs, bwd_stats=bs)
    (out * g).sum().backward()
    return dict(out=out.detach().cpu(), gy=yo.grad.cpu(), gp=torch.cat([p.grad.reshape(-1) for p in twin.parameters()]).cpu(),
                gt=to.grad.cpu(), fwd=fs, bwd=bs)


def at_err(got, ref):
    """max_i |got_i - ref_i| / max_i |ref_i| of a time gradient."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).abs().max() / ref.abs().max())


def adjoint_time_case(shape, grid, method='dopri5', mode='replay', arbiter=True):
    """Inputs and references of one case, computed once per process and left unchanged.

    Parameters: make_func(C, AT_SEED, kink_free=True).  The grid is rounded to fp32 (the ABI takes `float` times); the fp64 arbiter
    is given those values widened.  The cotangent makes grad_t WELL CONDITIONED: with a random dL/dy_i, <f_i, g_i> is a
    near-cancelling sum (|grad_t| ~ 0.2 against sum ||f_i|| ||g_i|| ~ 130) and a relative bound on it means nothing, so the fp32
    CPU oracle's forward solve supplies y(t_i), and g_i = noise_i + c_i ||noise_i|| f_i / ||f_i|| with c = AT_ALIGN and
    noise_i = randn / sqrt(C H W): every <f_i, g_i> is then a fixed fraction of ||f_i|| ||g_i||.

    Returns dict(shape, times (host floats of the fp32 grid), y, g [T, N, C, H, W], options, o32 = the fp32 CPU oracle's solve,
    f64 = the fp64 arbiter's on _arbiter_device() (arbiter=True), d32 = at_err(o32 grad_t, f64 grad_t), cond = min_i |grad_t_i| /
    sum_j ||f_j|| ||g_j|| over the arbiter's (else the oracle's) grad_t)."""
    from oracle import torchdiffeq_restated as tdq
    key = (tuple(shape), tuple(grid), method, mode)
    hit = _AT_CASES.get(key)
    if hit is not None and (hit['f64'] is not None or not arbiter):
        return hit
    N, C, H, W = shape
    T = len(grid)
    assert T <= len(AT_ALIGN)
    _, twin = make_func(C, seed=AT_SEED, kink_free=True)
    gen = torch.Generator().manual_seed(AT_SEED + 1)
    y = torch.randn(N, C, H, W, generator=gen)
    noise = torch.randn(T, N, C, H, W, generator=gen) / (C * H * W) ** 0.5
    t32 = torch.tensor(grid, dtype=torch.float32)
    options = at_options(method, mode)
    fopts = {'forced_dts': list(options['forced_dts'])} if options else None
    with torch.no_grad():
        traj = tdq.odeint(twin, y, t32, rtol=AT_TOL, atol=AT_TOL, method=method, options=fopts)
        fs = torch.stack([twin(t32[i], traj[i]) for i in range(T)])
    g = torch.stack([noise[i] + AT_ALIGN[i] * noise[i].norm() * fs[i] / fs[i].norm() for i in range(T)])
    o32 = _at_oracle(twin, y, t32, g, method, options)
    f64 = None
    if arbiter:
        dev = _arbiter_device()
        tw = copy.deepcopy(twin).to(torch.float64).to(dev)
        f64 = _at_oracle(tw, y.to(torch.float64).to(dev), t32.to(torch.float64).to(dev), g.to(torch.float64).to(dev), method, options)
    ref_gt = (f64 or o32)['gt'].double()
    scale = float(sum(fs[i].double().norm() * g[i].double().norm() for i in range(T)))
    case = dict(shape=tuple(shape), times=[float(v) for v in t32.tolist()], y=y, g=g, method=method, options=options, o32=o32, f64=f64,
                d32=at_err(o32['gt'], f64['gt']) if f64 else None, cond=float(ref_gt.abs().min()) / scale)
    _AT_CASES[key] = case
    return case


_AT_FUNCS = {}


def at_hip_solve(case, want_grad_t=True, grad_last_only=False, grad_out=None):
    """The library's forward and adjoint solve of a case through integrate.solve_forward / solve_adjoint (no autograd in between:
    the autograd surface discards grad_t).  `grad_out` replaces the case's cotangent; with `grad_last_only` it is the last slice
    alone.  Returns dict(out, gy, gp, gt (None unless wanted), fwd, bwd (the solves' statistics), pair (node_w4_pair_stats))."""
    from neural_ode_features_amd import _lib, integrate
    C = case['shape'][1]
    if C not in _AT_FUNCS:
        _AT_FUNCS[C] = make_func(C, seed=AT_SEED, device='cuda', kink_free=True)[0]
    f = _AT_FUNCS[C]
    rec = integrate.Recognised(f)
    mid = _lib.METHODS[case['method']]
    g = case['g'] if grad_out is None else grad_out
    with tune_env(NODE_TUNE_W4_STATS='1'):
        out, fs = integrate.solve_forward(rec, rec.params, case['y'].cuda(), case['times'], AT_TOL, AT_TOL, mid, case['options'])
        gy, gp, gt, bs = integrate.solve_adjoint(rec, rec.params, out, g.cuda(), case['times'], AT_TOL, AT_TOL, mid, case['options'],
                                                 want_grad_t=want_grad_t, grad_last_only=grad_last_only)
        st = (ctypes.c_int32 * 4)()
        _lib.check(_lib.load().node_w4_pair_stats(st))
    return dict(out=out.cpu(), gy=gy.cpu(), gp=gp.cpu(), gt=gt.cpu() if gt is not None else None, fwd=fs, bwd=bs, pair=list(st))


# ---------------------------------------------------------------------------------------------------------------------------------
# the stem's kernel family through the C ABI with a workspace of the caller's own (tests/test_gpu_stem_gn_paths.py,
# tests/test_gpu_stem_geometry.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def stem_family_gpu_run(kind, dims, mod, order, x, cot, with_dx=False):
    """One forward and one backward of a node through the C ABI: outputs, gradients and the workspace's bytes, all on the CPU.
    kind 'stem': dims (n, in_ch, h, w, filters), node_stem_fwd / node_stem_bwd -- and with `with_dx` node_stem_bwd_dx behind them on
    the same workspace, into gradient tensors of its own ('dx', 'dxgrad00' ..., 'ws_bwd_dx').  kind 'trunk': dims (n, channels, h, w,
    blocks), node_trunk_fwd / node_trunk_bwd ('dx' always).  Workspace, outputs and gradients start as 0xFF bytes (NaN in fp32 and
    bf16); 'ws_fwd' / 'ws_bwd' are the WHOLE workspace behind the forward and behind the backward."""
    from neural_ode_features_amd import _lib
    C = ctypes
    lib = _lib.load()
    n, a, h, w, c = dims
    m = copy.deepcopy(mod).cuda()
    ps = [p.detach().contiguous() for p in order(m)]
    xg, cg = x.cuda(), cot.cuda()
    nan = lambda t: torch.full(t.shape, float('nan'), dtype=torch.float32, device='cuda')
    grads = [nan(p) for p in ps]
    out = nan(cg)
    stream = torch.cuda.current_stream().cuda_stream
    eps = float(m[1].norm1.eps if kind == 'stem' else m[0].norm1.eps)
    if kind == 'stem':
        shape = _lib.NodeStemShape(n, a, h, w, c, eps)
        nbytes = lib.node_stem_workspace_bytes(C.byref(shape))
    else:
        shape = _lib.NodeTrunkShape(n, a, h, w, c, eps)
        nbytes = lib.node_trunk_workspace_bytes(C.byref(shape), 1)
    assert nbytes > 0, lib.node_last_error()
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device='cuda')
    wsp = (ws.data_ptr() + 255) & ~255
    res = {}
    if kind == 'stem':
        struct = lambda ts: _lib.NodeStemParams(*[t.data_ptr() for t in ts])
        _lib.check(lib.node_stem_fwd(C.byref(shape), C.byref(struct(ps)), xg.data_ptr(), out.data_ptr(), wsp, nbytes, stream))
        torch.cuda.synchronize()
        res['ws_fwd'] = ws.cpu()
        _lib.check(lib.node_stem_bwd(C.byref(shape), C.byref(struct(ps)), xg.data_ptr(), cg.data_ptr(), C.byref(struct(grads)), wsp,
                                     nbytes, stream))
        if with_dx:
            torch.cuda.synchronize()
            res['ws_bwd'] = ws.cpu()
            dx, grads2 = nan(xg), [nan(p) for p in ps]
            _lib.check(lib.node_stem_bwd_dx(C.byref(shape), C.byref(struct(ps)), xg.data_ptr(), cg.data_ptr(), C.byref(struct(grads2)),
                                            dx.data_ptr(), wsp, nbytes, stream))
            torch.cuda.synchronize()
            res['ws_bwd_dx'] = ws.cpu()
            res['dx'] = dx
            for i, g in enumerate(grads2):
                res['dxgrad%02d' % i] = g
    else:
        def blocks(ts):
            arr = (_lib.NodeTrunkBlock * c)()
            for i in range(c):
                arr[i] = _lib.NodeTrunkBlock(*[t.data_ptr() for t in ts[6 * i:6 * i + 6]])
            return arr
        dx = nan(xg)
        _lib.check(lib.node_trunk_fwd(C.byref(shape), blocks(ps), xg.data_ptr(), out.data_ptr(), None, 1, wsp, nbytes, stream))
        torch.cuda.synchronize()
        res['ws_fwd'] = ws.cpu()
        _lib.check(lib.node_trunk_bwd(C.byref(shape), blocks(ps), cg.data_ptr(), blocks(grads), dx.data_ptr(), wsp, nbytes, stream))
        res['dx'] = dx
    torch.cuda.synchronize()
    if 'ws_bwd' not in res:
        res['ws_bwd'] = ws.cpu()
    res['out'] = out
    for i, g in enumerate(grads):
        res['grad%02d' % i] = g
    return {k: v.cpu() for k, v in res.items()}

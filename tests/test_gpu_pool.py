"""GPU: the `ode` stem's hand-off -- nn.MaxPool2d(4, 2, 1) between its two solves (model.py:181-196) and the plane means of the
stem's trajectory in feature extraction -- as kernels of the library (neural_ode_features_amd/pool.py, csrc/kernels_pool.hip):
forward, argmax and backward bit for bit against ATen on the CPU (ties, NaN and -inf included), the means against fp64,
bit-reproducibility, the dispatch rules, one training step of an `ode` net with the pool fused and not, and the feature
extraction of the committed `ode` fixture net with the pool fused and not."""
import contextlib
import copy
import io
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (n, c, h, w): the fixture width; an odd side and an odd channel count; non-square with unaligned rows; a window that is all
# border; the workload's plane; the largest plane
CASES = [(3, 16, 16, 16), (2, 65, 7, 7), (1, 3, 5, 9), (2, 8, 2, 2), (4, 256, 16, 16), (2, 64, 32, 32)]
KINDS = ['randn', 'ties']


def _input(case, kind, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + sum(case))
    if kind == 'ties':
        return torch.randint(0, 3, case, generator=gen).float()       # ties everywhere
    return torch.randn(case, generator=gen)


def _flat_index(argmax):
    """the uint8 tap kh * 4 + kw of every output, decoded to the flat index h * W + w that `return_indices=True` reports"""
    a = argmax.cpu().long()
    oh = torch.arange(a.shape[-2]).view(1, 1, -1, 1)
    ow = torch.arange(a.shape[-1]).view(1, 1, 1, -1)
    return a, oh, ow


def _check_pool(x, equal_nan=False):
    """forward, argmax and backward of the fused node on `x` (CPU tensor) against ATen on the CPU; returns the GPU results"""
    from neural_ode_features_amd import pool
    n, c, h, w = x.shape
    xg = x.cuda().requires_grad_(True)
    y = pool.max_pool_4s2(xg)
    assert type(y.grad_fn).__name__ == '_MaxPool4s2FnBackward'           # the fused node, not F.max_pool2d
    xc = x.clone().requires_grad_(True)
    ref, idx = F.max_pool2d(xc, 4, 2, 1, return_indices=True)
    assert y.shape == ref.shape
    if equal_nan:
        assert torch.equal(torch.isnan(y.cpu()), torch.isnan(ref))
        assert torch.equal(torch.nan_to_num(y.detach().cpu(), nan=0.0), torch.nan_to_num(ref.detach(), nan=0.0))
    else:
        assert torch.equal(y.detach().cpu(), ref.detach())
    _, argmax, _ = pool._fwd(xg.detach(), (1,) + tuple(xg.shape), True, False)
    a, oh, ow = _flat_index(argmax)
    assert int(a.max()) <= 15
    assert torch.equal((2 * oh - 1 + a // 4) * w + (2 * ow - 1 + a % 4), idx)
    gen = torch.Generator().manual_seed(7 + n + c + h + w)
    gy = torch.randn(ref.shape, generator=gen)
    dx, = torch.autograd.grad(y, xg, gy.cuda(), retain_graph=True)
    dref, = torch.autograd.grad(ref, xc, gy)
    assert torch.equal(dx.cpu(), dref)
    dx2, = torch.autograd.grad(y, xg, gy.cuda())                         # a second backward through the same forward just runs
    assert torch.equal(dx2, dx)
    return y.detach(), argmax, dx


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_pool_matches_aten_bit_for_bit(case, kind):
    x = _input(case, kind)
    y, argmax, dx = _check_pool(x)
    y2, argmax2, dx2 = _check_pool(x)                                    # two runs: the same bits
    assert torch.equal(y, y2) and torch.equal(argmax, argmax2) and torch.equal(dx, dx2)


def test_pool_nan_and_minus_inf():
    """a NaN wins its windows and propagates; planes of -inf give -inf and name the first tap inside the image"""
    x = _input((2, 65, 7, 7), 'randn', seed=1)
    x.view(-1)[::11] = float('nan')
    _check_pool(x, equal_nan=True)
    x = _input((3, 16, 16, 16), 'ties', seed=1)
    x.view(-1)[::5] = float('nan')                                       # several NaNs per window: the last one is named
    _check_pool(x, equal_nan=True)
    x = _input((3, 16, 16, 16), 'randn', seed=2)
    x[:, ::2] = float('-inf')                                            # whole planes
    x[0, 1, :3] = float('-inf')                                          # and windows that are partly -inf
    y, _, _ = _check_pool(x, equal_nan=True)
    assert bool(torch.isinf(y[:, ::2]).all())
    x = _input((1, 3, 5, 9), 'randn', seed=3)
    x[0, 0] = float('-inf')
    x[0, 1, 2, 3] = float('nan')
    _check_pool(x, equal_nan=True)


def _mean_bound(traj):
    """|got - fp64 mean| <= H W 2^-24 mean|x| elementwise: the first-order bound of any fp32 summation order of H W terms plus the
    final division"""
    t64 = traj.double()
    h, w = traj.shape[-2:]
    return t64.mean((-1, -2)), h * w * 2.0 ** -24 * t64.abs().mean((-1, -2))


@pytest.mark.parametrize('t', [1, 4, 21])
@pytest.mark.parametrize('plane', [(2, 16, 16, 16), (2, 65, 7, 7)], ids=['2x16x16x16', '2x65x7x7'])
def test_trajectory_pool(t, plane):
    from neural_ode_features_amd import pool
    gen = torch.Generator().manual_seed(31 * t + sum(plane))
    traj = torch.randn((t,) + plane, generator=gen) + 100.0              # a dropped or double-counted column moves a mean by ~100 / W
    tg = traj.cuda()
    assert pool.fusable(tg)
    means, last = pool.trajectory_pool(tg)
    assert means.shape == (t,) + plane[:2] and means.dtype == torch.float32
    assert torch.equal(last.cpu(), F.max_pool2d(traj[-1], 4, 2, 1))
    ref, bound = _mean_bound(traj)
    err = (means.cpu().double() - ref).abs()
    print('trajectory_pool T=%d %s: worst mean error / bound %.3f' % (t, plane, float((err / bound).max())))
    assert bool((err <= bound).all())
    means2, last2 = pool.trajectory_pool(tg)
    assert torch.equal(means, means2) and torch.equal(last, last2)
    # ties in the last slice, and the other slices must not leak into the pool
    tied = torch.randint(0, 3, (t,) + plane, generator=gen).float()
    tied[:-1] += 50.0
    means, last = pool.trajectory_pool(tied.cuda())
    assert torch.equal(last.cpu(), F.max_pool2d(tied[-1], 4, 2, 1))
    ref, bound = _mean_bound(tied)
    assert bool(((means.cpu().double() - ref).abs() <= bound).all())


def test_dispatch():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import pool
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 16, 16, generator=gen).cuda()
    fused = nof.max_pool_4s2(x.clone().requires_grad_(True))
    assert type(fused.grad_fn).__name__ == '_MaxPool4s2FnBackward'
    with torch.no_grad():
        assert nof.max_pool_4s2(x).grad_fn is None and torch.equal(nof.max_pool_4s2(x), fused)
    # half precision: the module path, the same maxima
    xh = x.half().requires_grad_(True)
    assert not pool.fusable(xh)
    yh = nof.max_pool_4s2(xh)
    assert yh.dtype == torch.float16 and type(yh.grad_fn).__name__ != '_MaxPool4s2FnBackward'
    assert torch.equal(yh.float(), nof.max_pool_4s2(xh.detach().float()))
    # a view that is not contiguous
    xt = x.transpose(2, 3)
    assert not pool.fusable(xt) and torch.equal(nof.max_pool_4s2(xt), nof.max_pool_4s2(xt.contiguous()))
    # a trajectory that requires grad: the module path, differentiable, and the values of the fused path
    traj = (torch.randn(3, 2, 16, 16, 16, generator=gen) + 100.0).cuda()
    tr = traj.clone().requires_grad_(True)
    means_m, last_m = nof.trajectory_pool(tr)
    assert means_m.grad_fn is not None and last_m.grad_fn is not None
    means_f, last_f = nof.trajectory_pool(traj)
    assert means_f.grad_fn is None and torch.equal(last_f, last_m.detach())
    _, bound = _mean_bound(traj.cpu())
    assert bool(((means_f - means_m.detach()).abs().cpu().double() <= 2 * bound).all())      # each within `bound` of the fp64 mean
    # the stem's switch
    torch.manual_seed(6)
    stem = nof.ODEDownsample(3, 16).cuda()
    h = torch.randn(2, 16, 16, 16, generator=gen).cuda().requires_grad_(True)
    on = stem._pool(h)
    stem.fused_pool = False
    off = stem._pool(h)
    assert type(on.grad_fn).__name__ == '_MaxPool4s2FnBackward' and type(off.grad_fn).__name__ != '_MaxPool4s2FnBackward'
    assert torch.equal(on, off)
    gy = torch.randn(on.shape, generator=gen).cuda()
    g_on, = torch.autograd.grad(on, h, gy)
    g_off, = torch.autograd.grad(off, h, gy)
    # the module path's backward adds a pixel's (at most four) gradients with atomics, in any order: each sum is within
    # 3 * 2^-24 * sum|terms| of the exact one
    assert float((g_on - g_off).abs().max()) <= 2 * 3 * 2.0 ** -24 * 4 * float(gy.abs().max())


@pytest.fixture
def calls(monkeypatch):
    """the input shapes of every launch of the pool forward while the test runs, with what it was asked for"""
    from neural_ode_features_amd import pool
    seen = []
    real = pool._fwd
    monkeypatch.setattr(pool, '_fwd', lambda x, shape5, a, m: (seen.append((tuple(shape5), bool(a), bool(m))), real(x, shape5, a, m))[1])
    return seen


def test_ode_training_step_fused_and_module_pool_agree(calls):
    """`ODENet(downsample='ode')` at 64 filters on [8, 3, 32, 32] (states of 16x16 and 8x8): one training step with the fused pool
    and one with nn.MaxPool2d, from the same weights -- logits equal bit for bit (the forward is exact), equal NFE forward and
    backward for both blocks, worst per-tensor gradient error < 2e-2 (bound and scale formula of
    test_ode2_training_step_fused_and_module_handoff_agree; the module path's backward adds with atomics, which is what
    differs).  Kink-free weights as there: every GroupNorm bias in front of a ReLU at +8."""
    import neural_ode_features_amd as nof
    tol = 1e-3
    torch.manual_seed(17)
    net = nof.ODENet(3, out=10, n_filters=64, downsample='ode', method='dopri5', tol=tol, adjoint=True, t1=1, dropout=0)
    with torch.no_grad():
        for name, p in net.named_parameters():
            relu_behind = ('odefunc.norm' in name and 'norm3' not in name) or name == 'classifier.module.0.bias'
            if relu_behind and name.endswith('bias'):
                p.add_(8.0)
    twin = copy.deepcopy(net)
    gen = torch.Generator().manual_seed(18)
    x = torch.randn(8, 3, 32, 32, generator=gen).cuda()
    y = torch.randint(0, 10, (8,), generator=gen).cuda()
    runs = []
    for m, fused in ((net, True), (twin, False)):
        m = m.cuda().train()
        m.downsample.fused_pool = fused
        p = m(x)
        assert calls == [((1, 8, 64, 16, 16), True, False)]       # one fused pool in the first run, none in the second
        loss = F.cross_entropy(p, y)
        nfe_f = (m.downsample.odeblock.nfe, m.nfe())
        loss.backward()
        nfe_b = (m.downsample.odeblock.nfe - nfe_f[0], m.nfe() - nfe_f[1])
        runs.append((p.detach().cpu(), nfe_f, nfe_b, {k: v.grad.detach().cpu() for k, v in m.named_parameters()}))
    (p1, f1, b1, g1), (p0, f0, b0, g0) = runs
    print('ode step: nfe fused %s %s, modules %s %s, logits diff %.2e' % (f1, b1, f0, b0, float((p1 - p0).abs().max())))
    assert torch.equal(p1, p0)
    assert f1 == f0 and b1 == b0
    assert min(f1) > 0 and min(b1) > 0
    gmax = max(float(v.abs().max()) for v in g0.values())
    errs = {k: float((g1[k] - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * gmax) for k, ref in g0.items()}
    worst = max(errs, key=errs.get)
    print('ode step: worst per-tensor gradient error %.2e (%s)' % (errs[worst], worst))
    assert errs[worst] < 2e-2, (worst, errs[worst])


def test_ode_feature_extraction_fused_and_module_pool_agree(calls):
    """The net of tests/golden/odenet_ode_features.pt as a feature extractor, fused against `fused_pool = False`: ONE pool launch
    yields the stem's means and the continuation; the second block's features are bit-equal (its input is), the stem's means are
    within the summation bound of the fp64 means, NFE is equal."""
    import neural_ode_features_amd as nof
    g = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'odenet_ode_features.pt'), weights_only=False)
    with contextlib.redirect_stdout(io.StringIO()):
        net = nof.ODENet(3, out=10, n_filters=g['filters'], downsample='ode', tol=g['tol'], adjoint=True, t1=g['t1'])
    net.to_features_extractor()
    net.load_state_dict(g['state_dict'])
    net = net.cuda().eval()
    x = g['x'].cuda()
    res = {}
    for fused in (True, False):
        net.downsample.fused_pool = fused
        net.downsample.odeblock.nfe = 0
        net.nfe(reset=True)
        del calls[:]
        with torch.no_grad():
            stem = net.downsample(x, with_means=True)
            assert calls == ([((stem[0].shape), False, True)] if fused else [])       # means + pool: one launch
            assert (stem.means is not None) == fused
            feats = net(x)
        res[fused] = (stem, feats, (net.downsample.odeblock.nfe, net.nfe()))
    (s1, f1, n1), (s0, f0, n0) = res[True], res[False]
    assert n1 == n0
    traj = s0[0]
    assert torch.equal(s1[0], traj)                          # the same solve
    assert torch.equal(s1[1], s0[1])                         # the continuation
    t = traj.shape[0]
    assert f1.shape == f0.shape == g['features'].shape
    assert torch.equal(f1[t:], f0[t:])                       # the second block's features
    assert torch.equal(f1[:t], s1.means)                     # forward has not pooled again
    ref, bound = _mean_bound(traj.cpu())
    err = (s1.means.cpu().double() - ref).abs()
    print('ode features: worst stem mean error / bound %.3f' % float((err / bound).max()))
    assert bool((err <= bound).all())
    assert torch.allclose(f1.cpu(), g['features'], rtol=1e-3, atol=2e-4)

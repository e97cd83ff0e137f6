"""GPU: the `ode2` stem's hand-off -- GroupNorm -> ReLU -> Conv2d(cin, cout, 4, 2, 1) (model.py:199-223, `conv2(norm(x))`) -- as
one node of the library (neural_ode_features_amd/downconv.py, csrc/downconv_api.hip): output, input gradient and the four
parameter gradients against the same modules in fp64 on the CPU and against the reference's own modules
(tests/golden/ode2_handoff_c64.pt), bit-reproducibility, the stacked trajectory of `apply_conv`, the dispatcher trace, and one
training step of an `ode2` net with the hand-off fused and not."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

# (n, cin, cout, h, w): the MNIST hand-off, the CIFAR hand-off at 256 filters, an odd side with cin != cout, a non-square image
CASES = [(3, 64, 64, 14, 14), (8, 256, 256, 16, 16), (2, 64, 256, 15, 15), (5, 128, 128, 8, 6)]


def _pair(cin, cout, seed, kink_free=False):
    """(GroupNorm, Conv2d) as `ODEDownsample2` builds them, GroupNorm parameters perturbed as tests/test_gpu_stem.py::_stem_pair
    does, and their fp64 copies"""
    torch.manual_seed(seed)
    gn, conv = nn.GroupNorm(min(32, cin), cin), nn.Conv2d(cin, cout, 4, 2, 1)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in (gn.weight, gn.bias):
            p.add_(0.2 * torch.randn(p.shape, generator=gen))
        if kink_free:
            gn.bias.add_(8.0)          # every pre-activation positive: no ReLU mask can differ between fp32 and fp64
    return (gn, conv), (copy.deepcopy(gn).double(), copy.deepcopy(conv).double())


@pytest.fixture
def calls(monkeypatch):
    """the input shapes of every call of the fused node while the test runs"""
    from neural_ode_features_amd import downconv
    seen = []
    real = downconv._DownConvFn.apply
    monkeypatch.setattr(downconv._DownConvFn, 'apply', lambda *a: (seen.append(tuple(a[0].shape)), real(*a))[1])
    return seen


def _rel(a, b):
    return float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max())


def _run(case, seed=0, kink_free=False):
    from neural_ode_features_amd.downconv import gn_relu_conv
    n, cin, cout, h, w = case
    (gn, conv), (gn64, conv64) = _pair(cin, cout, seed=cin + cout + h + seed, kink_free=kink_free)
    gn, conv = gn.cuda(), conv.cuda()
    gen = torch.Generator().manual_seed(99 + n)
    x = torch.randn(n, cin, h, w, generator=gen)
    xg = x.cuda().requires_grad_(True)
    out = gn_relu_conv(xg, gn, conv)
    assert type(out.grad_fn).__name__ == '_DownConvFnBackward'          # the fused node, not the module sequence
    xd = x.double().requires_grad_(True)
    out_ref = conv64(F.relu(gn64(xd)))
    assert out.shape == out_ref.shape
    cot = torch.randn(out_ref.shape, generator=gen)
    out.backward(cot.cuda())
    out_ref.backward(cot.double())
    errs = {'out': _rel(out, out_ref), 'd_x': _rel(xg.grad, xd.grad),
            'gn.weight': _rel(gn.weight.grad, gn64.weight.grad), 'gn.bias': _rel(gn.bias.grad, gn64.bias.grad),
            'conv.weight': _rel(conv.weight.grad, conv64.weight.grad), 'conv.bias': _rel(conv.bias.grad, conv64.bias.grad)}
    got = [out.detach(), xg.grad, gn.weight.grad, gn.bias.grad, conv.weight.grad, conv.bias.grad]
    return errs, [g.clone() for g in got]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d_c%d-%d_%dx%d' % c)
def test_handoff_matches_fp64_and_is_reproducible(case):
    """Max-norm parity with the fp64 modules at the whole-stem bounds of tests/test_gpu_stem.py (2e-5 of the largest entry), and
    two runs that agree bit for bit in every output."""
    errs, first = _run(case)
    for k, e in errs.items():
        print('hand-off %s: %-12s max error / max|ref| = %.2e' % (case, k, e))
    _, second = _run(case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert max(errs.values()) <= 2e-5, errs


def test_handoff_matches_the_reference_fixture(golden_dir):
    """tests/golden/ode2_handoff_c64.pt: the reference's own `ODEDownsample2(1, 64).norm` / `.conv2` (model.py:199-223, imported
    by tests/golden/make_golden_convstem.py) on a [2, 64, 14, 14] input.  Their state_dicts load unchanged."""
    import neural_ode_features_amd as nof
    g = torch.load(os.path.join(golden_dir, 'ode2_handoff_c64.pt'), map_location='cpu', weights_only=False)
    stem = nof.ODEDownsample2(1, 64)
    stem.norm.load_state_dict(g['norm'])
    stem.conv2.load_state_dict(g['conv2'])
    stem = stem.cuda()
    x = g['x'].cuda().requires_grad_(True)
    out = stem._handoff(x)
    assert type(out.grad_fn).__name__ == '_DownConvFnBackward'
    out.backward(g['cot'].cuda())
    err = float((out.detach().cpu() - g['out']).abs().max() / g['out'].abs().max())
    print('reference hand-off fixture: output max error / max|ref| = %.2e' % err)
    assert err <= 2e-5
    named = dict(stem.named_parameters())
    for name, ref in list(g['grads'].items()) + [('d_x', g['d_x'])]:
        got = x.grad if name == 'd_x' else named[name].grad
        e = float((got.cpu() - ref).abs().max() / ref.abs().max())
        print('  grad %-16s %.2e' % (name, e))
        assert e <= 1e-4, (name, e)       # (the fixture itself is fp32: PyTorch-CPU's own rounding sits at ~1e-6)


def test_trajectory_is_one_call_and_equals_the_slices(calls, monkeypatch):
    """`apply_conv`: the [T = 3, N = 2] trajectory goes through the hand-off as ONE batch of T N samples (GroupNorm is per
    sample), and every slice has the bits of its own call."""
    import neural_ode_features_amd as nof
    torch.manual_seed(5)
    stem = nof.ODEDownsample2(3, 64, tol=1e-3).cuda().eval()
    stem.apply_conv = True
    traj = torch.randn(3, 2, 64, 16, 16, device='cuda')
    monkeypatch.setattr(stem.odeblock, 'forward', lambda x: traj)     # the trajectory a solve with three output times returns
    with torch.no_grad():
        y, last = stem(torch.randn(2, 3, 32, 32, device='cuda'))
    assert calls == [(6, 64, 16, 16)], calls
    assert y.shape == (3, 2, 64, 8, 8) and torch.equal(last, y[-1])
    with torch.no_grad():
        for i in range(3):
            assert torch.equal(y[i], stem._handoff(traj[i])), i
    stem.apply_conv = False                     # the last slice alone
    with torch.no_grad():
        normed, last2 = stem(torch.randn(2, 3, 32, 32, device='cuda'))
    assert normed.shape == traj.shape and torch.equal(last2, y[-1])


def test_handoff_runs_no_library_convolution():
    """ONE autograd node whose forward and backward are calls into libnode_hip.so: the dispatcher trace of a forward + backward
    holds no convolution, GroupNorm, ReLU or transpose operator (the check of test_stem_runs_no_library_convolution)."""
    from torch.profiler import ProfilerActivity, profile
    from neural_ode_features_amd.downconv import gn_relu_conv
    (gn, conv), _ = _pair(256, 256, seed=7)
    gn, conv = gn.cuda(), conv.cuda()
    x = torch.randn(8, 256, 16, 16, device='cuda', requires_grad=True)
    gn_relu_conv(x, gn, conv).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        out = gn_relu_conv(x, gn, conv)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('conv', 'miopen', 'group_norm', 'native_group_norm', 'transpose', 'relu'))
           and '_DownConvFn' not in k]
    assert not bad, bad
    assert any('_DownConvFn' in k for k in names), names


def test_handoff_falls_back_to_the_modules(calls):
    """What the kernels do not take runs the modules and still matches fp64: 32 channels, a convolution without bias; a forward
    under no_grad stays fused (on the forward-only workspace)."""
    from neural_ode_features_amd.downconv import gn_relu_conv
    (gn, conv), (gn64, conv64) = _pair(32, 32, seed=3)
    gn, conv = gn.cuda(), conv.cuda()
    x = torch.randn(2, 32, 14, 14)
    out = gn_relu_conv(x.cuda().requires_grad_(True), gn, conv)
    assert type(out.grad_fn).__name__ != '_DownConvFnBackward' and not calls
    assert _rel(out, conv64(F.relu(gn64(x.double())))) <= 1e-4
    (gn, conv), (gn64, conv64) = _pair(64, 64, seed=4)
    gn, conv = gn.cuda(), conv.cuda()
    x = torch.randn(2, 64, 14, 14)
    with torch.no_grad():
        out = gn_relu_conv(x.cuda(), gn, conv)
    assert calls == [(2, 64, 14, 14)] and out.grad_fn is None and _rel(out, conv64(F.relu(gn64(x.double())))) <= 2e-5
    nobias = nn.Conv2d(64, 64, 4, 2, 1, bias=False).cuda()
    out = gn_relu_conv(x.cuda(), gn, nobias)
    assert type(out.grad_fn).__name__ != '_DownConvFnBackward' and len(calls) == 1


def test_ode2_training_step_fused_and_module_handoff_agree(calls):
    """`ODENet(downsample='ode2')` at 64 filters on [8, 3, 32, 32] (states of 16x16 and 8x8): one training step with the fused
    hand-off and one with the module path, from the same weights -- equal NFE forward and backward for both blocks, logits
    within 10 tol, worst per-tensor gradient error < 2e-2 (bounds and scale formula of test_ode_stem_fixtures_on_gpu).  This
    catches wiring mistakes; the numerics are pinned by the cases above.

    The weights are kink-free (every GroupNorm bias in front of a ReLU at +8, as in test_three_stacked_blocks): the two runs'
    hand-offs differ by fp32 rounding (logits by 2.4e-7), and with ordinary weights that is enough to flip the ReLU mask of one
    or two of the ~10 M pre-activations the two solves evaluate, each of which moves a GroupNorm-bias gradient entry (a sum over
    8 x 256 terms of random sign) by ~2e-2: two runs of the same code measured a worst error below 2e-2 and of 3.9e-2."""
    import neural_ode_features_amd as nof
    tol = 1e-3
    torch.manual_seed(17)
    net = nof.ODENet(3, out=10, n_filters=64, downsample='ode2', method='dopri5', tol=tol, adjoint=True, t1=1, dropout=0)
    with torch.no_grad():
        for name, p in net.named_parameters():
            relu_behind = ('odefunc.norm' in name and 'norm3' not in name) or name in ('downsample.norm.0.bias', 'classifier.module.0.bias')
            if relu_behind and name.endswith('bias'):
                p.add_(8.0)
    twin = copy.deepcopy(net)
    gen = torch.Generator().manual_seed(18)
    x = torch.randn(8, 3, 32, 32, generator=gen).cuda()
    y = torch.randint(0, 10, (8,), generator=gen).cuda()
    runs = []
    for m, fused in ((net, True), (twin, False)):
        m = m.cuda().train()
        m.downsample.fused_handoff = fused
        p = m(x)
        assert calls == [(8, 64, 16, 16)]              # one fused hand-off in the first run, none in the second
        loss = F.cross_entropy(p, y)
        nfe_f = (m.downsample.odeblock.nfe, m.nfe())
        loss.backward()
        nfe_b = (m.downsample.odeblock.nfe - nfe_f[0], m.nfe() - nfe_f[1])
        runs.append((p.detach().cpu(), nfe_f, nfe_b, {k: v.grad.detach().cpu() for k, v in m.named_parameters()}))
    (p1, f1, b1, g1), (p0, f0, b0, g0) = runs
    print('ode2 step: nfe fused %s %s, modules %s %s, logits diff %.2e' % (f1, b1, f0, b0, float((p1 - p0).abs().max())))
    assert f1 == f0 and b1 == b0
    assert float((p1 - p0).abs().max()) <= 10 * tol
    gmax = max(float(v.abs().max()) for v in g0.values())
    errs = {k: float((g1[k] - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * gmax) for k, ref in g0.items()}
    worst = max(errs, key=errs.get)
    print('ode2 step: worst per-tensor gradient error %.2e (%s)' % (errs[worst], worst))
    assert errs[worst] < 2e-2, (worst, errs[worst])

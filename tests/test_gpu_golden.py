"""GPU: the HIP path against the fixtures generated from the REFERENCE's own modules
(tests/golden/), and size-independent properties at BASELINE.json's full sizes."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import make_func, rel_err, robust_grad_err

pytestmark = pytest.mark.gpu


def _load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location='cpu', weights_only=False)


@pytest.mark.parametrize('name', ['odefunc_c8.pt', 'odefunc_c16.pt', 'odefunc_c64.pt'])
def test_hip_dynamics_match_reference_odefunc_fixture(golden_dir, name):
    import neural_ode_features_amd as nof
    g = _load(golden_dir, name)
    f = nof.ODEfunc(g['C'])
    f.load_state_dict(g['state_dict'])            # reference state_dict loads unchanged
    f = f.cuda()
    fo, vy, vt, vp = nof.odefunc_vjp(f, float(g['t']), g['y'].cuda(), g['cotangent'].cuda())
    assert rel_err(fo, g['f']) < 1e-5              # <= 1e-6-class agreement with the reference ODEfunc
    assert rel_err(vy, g['vjp_y']) < 2e-5
    assert rel_err(vp, g['vjp_params']) < 2e-5
    assert abs(float(vt) - float(g['vjp_t'])) < 2e-5 * max(1.0, abs(float(g['vjp_t'])))
    assert rel_err(nof.odefunc_forward(f, float(g['t']), g['y'].cuda()), g['f']) < 1e-5


@pytest.mark.parametrize('name', ['odenet_rk4.pt', 'odenet_dopri5.pt', 'odenet_rk4_f64.pt'])
def test_hip_end_to_end_matches_reference_run(golden_dir, name):
    """Reference ODENet + oracle solver (fixture)  vs  package ODENet + HIP solver.  `odenet_rk4_f64.pt` is the model of
    BASELINE.json configs[0] (64 filters, MNIST-shaped input, rk4, adjoint): the stem runs on the library's own kernels there."""
    import neural_ode_features_amd as nof
    g = _load(golden_dir, name)
    net = nof.ODENet(g['in_ch'], out=10, n_filters=g['filters'], downsample='residual', method=g['method'],
                     tol=g['tol'], adjoint=True, t1=g['t1'], dropout=0)
    net.load_state_dict(g['state_dict'])
    net = net.cuda().train()
    p = net(g['x'].cuda())
    loss = F.cross_entropy(p, g['y'].cuda())
    nfe_f = net.nfe(reset=True)
    loss.backward()
    nfe_b = net.nfe(reset=True)
    assert (nfe_f, nfe_b) == (g['nfe_f'], g['nfe_b'])            # same steps taken, same NFE accounting
    assert float((p.detach().cpu() - g['logits']).abs().max()) <= 10 * g['tol']
    assert rel_err(p, g['logits']) < 1e-3
    assert abs(float(loss) - float(g['loss'])) < 1e-4
    # With one channel per group (C=8 here) a conv bias in front of a GroupNorm, and norm3.bias in front
    # of the head's GroupNorm, have exactly-zero gradients; both sides then hold only rounding noise
    # (~1e-9 against a largest gradient of ~0.2), so each tensor is compared relative to
    # max(its own scale, 1e-4 x the largest gradient of the net).
    gmax = max(float(v.abs().max()) for v in g['grads'].values())
    # Stems of at least 64 filters run on this package's own kernels (stem.py, csrc/kernels_stem.hip) and are held to the
    # bound of the ODE block and the head; the toy widths of some fixtures (8, 16 filters) fall back to PyTorch's library
    # convolutions, whose backward kernels were measured to differ by up to 4e-3 relative between algorithm choices on a
    # fresh box (tests/test_gpu_head.py): those keep the wider bound.
    from neural_ode_features_amd import stem as stem_mod
    own_stem = isinstance(net.downsample.module, stem_mod.ResidualStem) and stem_mod.fusable(net.downsample.module, g['x'].cuda())
    assert own_stem == (g['filters'] >= 64)
    for k, v in net.named_parameters():
        ref = g['grads'][k]
        scale = max(float(ref.abs().max()), 1e-4 * gmax)
        bound = 2e-2 if (k.startswith('downsample') and not own_stem) else 5e-3
        assert float((v.grad.detach().cpu() - ref).abs().max()) / scale < bound, k


def test_cfg1_exact_shape_training_step_vs_oracle():
    """BASELINE.json configs[0] at its own size on the HIP path: MNIST-shaped batch [32, 1, 28, 28] ~ U[0, 1), `ODENet(1,
    n_filters=64, downsample='residual', method='rk4', adjoint=True)` (reproduce.sh:9) -- state [32, 64, 7, 7], one rk4 3/8
    step forward (NFE-F 4), one backward (NFE-B 5) -- one training step against the same net on the CPU with the oracle
    standing in for torchdiffeq.  Dropout off: the two devices' generators draw different masks."""
    import copy
    import neural_ode_features_amd as nof
    from oracle import torchdiffeq_restated as tdq
    torch.manual_seed(23)
    net = nof.ODENet(1, out=10, n_filters=64, downsample='residual', method='rk4', tol=1e-3, adjoint=True, t1=1, dropout=0)
    ref = copy.deepcopy(net)
    ref.odeblock.odeint = tdq.odeint_adjoint
    gen = torch.Generator().manual_seed(1)
    x = torch.rand(32, 1, 28, 28, generator=gen)
    y = torch.randint(0, 10, (32,), generator=gen)
    net = net.cuda().train()
    ref.train()
    p = net(x.cuda())
    assert type(net.downsample.module(x.cuda()).grad_fn).__name__ == '_StemFnBackward'     # own stem kernels at 64 filters
    loss = nof.cross_entropy(p, y.cuda())
    nfe_f = net.nfe(reset=True)
    loss.backward()
    nfe_b = net.nfe(reset=True)
    pr = ref(x)
    assert tuple(ref.odeblock.odefunc.norm1.weight.shape) == (64,) and pr.shape == (32, 10)
    lr = F.cross_entropy(pr, y)
    rf = ref.nfe(reset=True)
    lr.backward()
    rb = ref.nfe(reset=True)
    assert (nfe_f, nfe_b) == (rf, rb) == (4, 5)
    assert float((p.detach().cpu() - pr.detach()).abs().max()) <= 1e-4 and abs(float(loss) - float(lr)) < 1e-5
    gmax = max(float(v.grad.abs().max()) for v in ref.parameters())
    for (k, v), (_, r) in zip(net.named_parameters(), ref.named_parameters()):
        scale = max(float(r.grad.abs().max()), 1e-4 * gmax)
        assert float((v.grad.cpu() - r.grad).abs().max()) / scale < 5e-3, k


@pytest.fixture
def one_host_thread():
    """PyTorch-CPU on ONE thread for the test's duration.  Its fp32 reductions are split by the thread count, and a training
    trajectory amplifies that rounding: the oracle loop of the five-step test below, against one and the same GPU run, is
    1.18e-2 of a tensor's movement away at 1 and 4 threads, 6.8e-3 at 8, 4.3e-2 at 16.  Pinned, the reference is the same
    on every host instead of following its core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize('method,tol', [('rk4', 1e-3), ('dopri5', 1e-5)])
def test_five_step_training_trajectory_vs_oracle_loop(method, tol, one_host_thread):
    """A TRAJECTORY, not a step (round-5 review, rows A9 / f4): five SGD-with-momentum iterations of the reference's loop body
    (train.py:40-58: forward, cross-entropy, backward, optimizer.step) on the cfg-1 model -- `ODENet(1, n_filters=64, 'residual',
    adjoint)` on MNIST-shaped batches -- on the HIP path (own stem kernels, fused head / loss, `nof.FusedSGD`) against the same net
    on the CPU with the oracle standing in for torchdiffeq and `torch.optim.SGD`.  The two must stay together: loss of every
    iteration within 1e-4, evaluation counts equal, every parameter tensor's five-step movement within 3 % of itself.  Dropout
    off (the devices' generators differ).  rk4 = configs[0] itself; dopri5 (tol 1e-5) = the same model through the adaptive solver (7x7 states: the F(2x2,3x3) kernels)."""
    import copy
    import neural_ode_features_amd as nof
    from oracle import torchdiffeq_restated as tdq
    torch.manual_seed(29)
    net = nof.ODENet(1, out=10, n_filters=64, downsample='residual', method=method, tol=tol, adjoint=True, t1=1, dropout=0)
    ref = copy.deepcopy(net)
    ref.odeblock.odeint = tdq.odeint_adjoint
    net = net.cuda().train()
    ref.train()
    init = {k: v.detach().clone() for k, v in ref.named_parameters()}
    opt = nof.FusedSGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    opt_ref = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    gen = torch.Generator().manual_seed(2)
    for it in range(5):
        x = torch.rand(32, 1, 28, 28, generator=gen)
        y = torch.randint(0, 10, (32,), generator=gen)
        opt.zero_grad()
        loss = nof.cross_entropy(net(x.cuda()), y.cuda())
        nf = net.nfe(reset=True)
        loss.backward()
        nb = net.nfe(reset=True)
        opt.step()
        opt_ref.zero_grad()
        lr_ = F.cross_entropy(ref(x), y)
        rf = ref.nfe(reset=True)
        lr_.backward()
        rb = ref.nfe(reset=True)
        opt_ref.step()
        print('iteration %d (%s): loss %.6f | oracle loop %.6f; NFE %d / %d | %d / %d' % (it, method, float(loss.detach()), float(lr_.detach()), nf, nb, rf, rb))
        # (rk4: a fixed scheme, the two loops differ by rounding.  dopri5 runs at tol 1e-5: at 1e-3 both loops carry a solver error of the
        #  order of the tolerance that depends on rounding through the step sizes -- measured: losses 2e-4 apart at the fourth iteration,
        #  the first conv's weights 15 % of their movement apart after five -- which says nothing about either loop)
        assert abs(float(loss) - float(lr_)) < (1e-4 if method == 'rk4' else 2e-4), it
        assert (nf, nb) == (rf, rb), it
    # the five UPDATES agree: per tensor, the distance between the two trajectories against the largest movement of that tensor
    # (the single-step test above bounds a gradient's error by 5e-3 of its largest entry; momentum carries it through the steps)
    worst = 0.0
    for (k, v), (_, r) in zip(net.named_parameters(), ref.named_parameters()):
        moved = float((r.detach() - init[k]).abs().max())
        d = float((v.detach().cpu() - r.detach()).abs().max())
        worst = max(worst, d / max(moved, 1e-12))
        # (rk4, measured worst: 1.1e-2, a GroupNorm bias of the stem.  dopri5: ~60 + ~75 evaluations per iteration, each a chance for a
        #  ReLU mask to differ between two fp32 implementations: single gradient entries move by per cents)
        assert d <= (3e-2 if method == 'rk4' else 2e-1) * moved + 1e-7, (k, d, moved)
    print('largest trajectory distance / movement over the parameter tensors: %.2e' % worst)


def test_full_size_cifar_state_forward_and_vjp_vs_oracle():
    """BASELINE configs[1] state [128, 256, 8, 8]: one dynamics eval + VJP against the oracle.

    4.2 M pre-activations pass a ReLU here, so with generic parameters about one of them lies within fp32
    rounding of zero and its mask may flip between two correct implementations; GroupNorm's backward
    then spreads the difference over that one sample (measured: exactly one sample differs, the other
    127 agree to 1e-6).  The tight element-wise comparison therefore runs on the kink-free parameter
    set (helpers.make_func); the generic set is held to: forward tight, at most two samples affected,
    all others tight."""
    import neural_ode_features_amd as nof
    from oracle.dynamics import odefunc_vjp as oracle_vjp
    gen = torch.Generator().manual_seed(8)
    y = torch.randn(128, 256, 8, 8, generator=gen)
    cot = torch.randn(128, 256, 8, 8, generator=gen)

    f, twin = make_func(256, seed=2, device='cuda', kink_free=True)
    fo, vy, vt, vp = nof.odefunc_vjp(f, 0.5, y.cuda(), cot.cuda())
    f_ref, vy_ref, vt_ref, vp_ref = oracle_vjp(0.5, y, dict(twin.named_parameters()), cot)
    assert rel_err(fo, f_ref) < 2e-5 and rel_err(vy, vy_ref) < 5e-5 and rel_err(vp, vp_ref) < 5e-5
    assert abs(float(vt) - float(vt_ref)) < 1e-4 * abs(float(vt_ref)) + 1e-3
    # linearity of the VJP in the cotangent (size-independent property)
    _, vy2, vt2, vp2 = nof.odefunc_vjp(f, 0.5, y.cuda(), (-2.0 * cot).cuda())
    assert rel_err(vy2, -2.0 * vy) < 1e-5 and rel_err(vp2, -2.0 * vp) < 1e-5

    f, twin = make_func(256, seed=2, device='cuda')
    fo, vy, vt, vp = nof.odefunc_vjp(f, 0.5, y.cuda(), cot.cuda())
    f_ref, vy_ref, vt_ref, vp_ref = oracle_vjp(0.5, y, dict(twin.named_parameters()), cot)
    assert rel_err(fo, f_ref) < 2e-5
    per_sample = (vy.cpu() - vy_ref).abs().amax(dim=(1, 2, 3)) / float(vy_ref.abs().max())
    assert int((per_sample > 5e-5).sum()) <= 2, per_sample.topk(4)
    assert robust_grad_err(vp, vp_ref)[0] < 5e-2


def test_full_size_solve_properties():
    """configs[1]/[2] at full size: NFE law, y_out[0] == y0, sample independence under a
    forced step sequence (the only cross-sample coupling is the error norm), and agreement
    with the oracle within 10 x atol."""
    import neural_ode_features_amd as nof
    from oracle import torchdiffeq_restated as tdq
    f, twin = make_func(256, seed=4, device='cuda')
    y = torch.randn(128, 256, 8, 8, generator=torch.Generator().manual_seed(9))
    t = torch.tensor([0.0, 1.0])
    for tol in (1e-3, 1e-5):
        f.nfe = 0
        with torch.no_grad():
            out = nof.odeint(f, y.cuda(), t.cuda(), rtol=tol, atol=tol, method='dopri5')
        st = f.last_forward_stats
        assert f.nfe == 2 + 6 * (st['accepted'] + st['rejected'])
        assert torch.equal(out[0].cpu(), y)
        with torch.no_grad():
            want = tdq.odeint(twin, y, t, rtol=tol, atol=tol, method='dopri5')
        assert float((out[-1].cpu() - want[-1]).abs().max()) <= 10 * tol
    dts = [0.1, 0.25, 0.35, 0.4]
    with torch.no_grad():
        full = nof.odeint(f, y.cuda(), t.cuda(), rtol=1e-3, atol=1e-3, options={'forced_dts': dts})[-1]
        part = nof.odeint(f, y[5:37].cuda(), t.cuda(), rtol=1e-3, atol=1e-3, options={'forced_dts': dts})[-1]
        y2 = torch.randn(128, 256, 8, 8, generator=torch.Generator().manual_seed(19))
        big = nof.odeint(f, torch.cat([y, y2]).cuda(), t.cuda(), rtol=1e-3, atol=1e-3, options={'forced_dts': dts})[-1]
    # batch rows never mix: bit-identical where the same conv kernel serves both batches (128 and 256 samples:
    # the 2-D Winograd tile), to rounding where the small batch is served by another tiling (32 samples fill
    # too few workgroups for the 128-pixel tile, so the 64-pixel 1-D Winograd kernel runs instead)
    assert torch.equal(big[:128], full)
    assert float((full[5:37] - part).abs().max()) <= 2e-5 * float(full.abs().max())


def test_ragged_and_edge_shapes():
    """N not a multiple of the samples-per-tile, single sample, single time interval reversed."""
    import neural_ode_features_amd as nof
    from oracle import torchdiffeq_restated as tdq
    for shape in [(1, 64, 7, 7), (7, 64, 7, 7), (3, 8, 1, 1)]:
        N, C, H, W = shape
        f, twin = make_func(C, seed=13, device='cuda')
        y = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(10))
        t = torch.tensor([0.0, 1.0])
        with torch.no_grad():
            got = nof.odeint(f, y.cuda(), t.cuda(), rtol=1e-3, atol=1e-3, method='dopri5')
            want = tdq.odeint(twin, y, t, rtol=1e-3, atol=1e-3, method='dopri5')
        assert float((got[-1].cpu() - want[-1]).abs().max()) <= 1e-2, shape
    f, twin = make_func(16, seed=14, device='cuda')
    y = torch.randn(2, 16, 4, 4, generator=torch.Generator().manual_seed(11))
    t = torch.tensor([1.0, 0.25])                 # decreasing times: upstream negates t and f
    with torch.no_grad():
        got = nof.odeint(f, y.cuda(), t.cuda(), rtol=1e-4, atol=1e-4, method='dopri5')
        want = tdq.odeint(twin, y, t, rtol=1e-4, atol=1e-4, method='dopri5')
    assert float((got[-1].cpu() - want[-1]).abs().max()) <= 1e-3


def test_errors_surface_as_python_exceptions():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd._lib import NodeHipError
    f, _ = make_func(8, seed=1, device='cuda')
    y = torch.randn(2, 8, 4, 4).cuda()
    with pytest.raises(NodeHipError, match='MAX_STEPS'):
        nof.odeint(f, y, torch.tensor([0.0, 1.0]).cuda(), rtol=1e-9, atol=1e-9, options={'max_num_steps': 2})
    with pytest.raises(ValueError):
        nof.odeint(f, y, torch.tensor([0.0, 1.0, 0.5]).cuda())
    with pytest.raises(TypeError):
        nof.odeint(f, y.double(), torch.tensor([0.0, 1.0]).cuda())
    g, _ = make_func(16, seed=1, device='cuda')
    with pytest.raises(ValueError):
        nof.odeint(g, y, torch.tensor([0.0, 1.0]).cuda())          # channel mismatch
    from neural_ode_features_amd import integrate
    integrate.GENERIC_FALLBACK = False         # (with the fallback on, this geometry runs the generic solver: test_gpu_generic.py)
    try:
        with pytest.raises(NodeHipError, match='UNSUPPORTED'):
            nof.odeint(f, torch.randn(1, 8, 20, 20).cuda(), torch.tensor([0.0, 1.0]).cuda())
    finally:
        integrate.GENERIC_FALLBACK = True

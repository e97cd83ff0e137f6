"""GPU: the `ode2` stem's hand-off `conv2(norm(x))` with `norm='batch'` as one HIP node (downconv.py `_BnDownConvFn`,
csrc/bndownconv_api.hip: node_bndownconv_fwd / node_bndownconv_bwd; reference model.py:199-223 with model.py:274), the sliced call
that takes a whole trajectory slice by slice (model.py:214-216; the sliced BatchNorm passes of csrc/kernels_batchnorm.hip),
`ODEDownsample2(..., norm='batch')` on both, and the `-d ode2` command lines.

Reference: the same modules as `.double()` on the CPU (tests/bnconvstem_cases.py), never the node; a trajectory's reference runs them
slice by slice.  Metric: bntrunk_cases.errors.  Bound per quantity: max(2e-5, 4 x the same error of the fp32 modules on the CPU),
computed here -- tests/bnstem_cases.py's, unchanged.

Every run asserts `type(out.grad_fn).__name__ == '_BnDownConvFnBackward'`: without the node the modules run and every test built
on `run_node` fails.

Worst measured error per case on an MI355X (ordinary / kinkfree / split); bound 2e-5 where no other is given:
    (2, 64, 4)           5.6e-7 / 5.5e-7 / 7.4e-7        (2, 192, 8)          1.4e-6 / 1.4e-6 / 1.7e-6
    (2, 64, (7, 6))      7.3e-7 / 9.5e-7 / 6.4e-7        (2, 64 -> 128, 8)    6.9e-7 / 8.8e-7 / 1.3e-6
    (3, 128, 8)          9.0e-7 / 1.4e-6 / 9.8e-7        (9, 64, (24, 19))    8.2e-7 / 1.4e-6 / 1.3e-6
    (2, 256, 16)         1.7e-6 / 2.2e-6 / 2.5e-6
the worst quantity is the output everywhere but at (2, 64, 4) kinkfree (the input gradient); no gradient above 1.0e-6.
Sliced [3, 2, 64, 8, 8]: 9.1e-7 / 1.1e-6 / 1.3e-6; [3, 2, 64, 7, 6]: 9.3e-7 / 1.0e-6 / 6.6e-7 (the flattened batch with slices = 1 is off by
4.5e-2 .. 5.2e-1).  The hand-off of a trajectory with gradients (T calls): output 1.1e-6, parameter gradients at most 3.2e-7."""
import math
import os
from unittest import mock

import pytest
import torch
from torch import nn

from tests import bnconvstem_cases as K
from tests import bntrunk_cases as T

pytestmark = pytest.mark.gpu
NODE = '_BnDownConvFnBackward'


def _id(v):
    if isinstance(v, str):
        return v
    return '_'.join('%dx%d' % s if isinstance(s, tuple) else str(s) for s in v)


def _node(mod, x, slices=1):
    import neural_ode_features_amd as nof
    return nof.downconv.bn_relu_conv(x, mod[0], mod[2], slices)


def run_node(case, mode, frozen=False):
    """Forward + backward of the node on the GPU: (out, d_x, parameter gradients by name, ())."""
    seed = K.seed_of(case, mode)
    mod = K.module_pair(case, seed, mode)[0].cuda()
    if frozen:
        for p in mod.parameters():
            p.requires_grad_(False)
    x, cot = K.case_inputs(case, seed)
    xg = x.cuda().requires_grad_(True)
    out = _node(mod, xg)
    assert type(out.grad_fn).__name__ == NODE          # the node, not the modules
    out.backward(cot.cuda())
    return out.detach(), xg.grad, {k: p.grad for k, p in mod.named_parameters()}, ()


def check_against_fp64(case, mode, got):
    r64, r32 = K.references(case, mode)
    errs, floor = T.errors(got, r64), T.errors(r32, r64)
    assert len(errs) == 2 + 4
    bad = {}
    for k, v in errs.items():
        bnd = K.bound(floor[k])
        print('bndownconv %s %s: %-16s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (_id(case), mode, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    worst = max(errs, key=errs.get)
    print('bndownconv %s %s: WORST %s %.2e' % (_id(case), mode, worst, errs[worst]))
    assert not bad, bad


RUNS = [r for case in K.DOWN_ALL for r in K.runs(case)]


@pytest.mark.parametrize('case,mode', RUNS, ids=_id)
def test_output_input_gradient_and_every_parameter_gradient_match_fp64(case, mode):
    check_against_fp64(case, mode, run_node(case, mode))


def test_the_multi_chunk_case_reaches_its_regimes():
    from neural_ode_features_amd import _lib
    for case, asked in K.DOWN_MULTI.items():
        n, c, h, w = K.shape_of(case)
        d = _lib.describe_bndownconv(n, c, case[3], h, w)
        assert d['rows'] > 4096 and d['column_tiles'] == 1
        for regime in asked:
            assert K.REGIMES[regime](d), (case, regime, d)


def test_frozen_parameters_leave_the_input_gradient_bit_for_bit():
    case, mode = ('down', 9, 64, 64, (24, 19)), 'ordinary'
    full, frozen = run_node(case, mode), run_node(case, mode, frozen=True)
    assert torch.equal(full[0], frozen[0]) and torch.equal(full[1], frozen[1])
    assert all(g is None for g in frozen[2].values()) and all(g is not None for g in full[2].values())


def test_two_runs_return_the_same_bits():
    case, mode = ('down', 9, 64, 64, (24, 19)), 'kinkfree'
    a, b = run_node(case, mode), run_node(case, mode)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_forwards_in_flight_keep_their_own_workspaces_and_a_second_backward_raises():
    case = ('down', 2, 64, 128, 8)
    mod = K.module_pair(case, 2)[0].cuda()
    xs = [K.case_inputs(case, s)[0].cuda() for s in (1, 2, 3)]
    cots = [K.case_inputs(case, s)[1].cuda() for s in (1, 2)]

    def alone(i):
        for p in mod.parameters():
            p.grad = None
        x = xs[i].clone().requires_grad_(True)
        _node(mod, x).backward(cots[i])
        return x.grad, [p.grad.clone() for p in mod.parameters()]
    want = [alone(0), alone(1)]
    ins = [xs[i].clone().requires_grad_(True) for i in (0, 1)]
    outs = [_node(mod, ins[0])]
    with torch.no_grad():
        free = _node(mod, xs[2])
    outs.append(_node(mod, ins[1]))
    assert all(type(o.grad_fn).__name__ == NODE for o in outs) and free.grad_fn is None
    for i in (1, 0):
        for p in mod.parameters():
            p.grad = None
        outs[i].backward(cots[i], retain_graph=True)
        assert torch.equal(ins[i].grad, want[i][0])
        for p, g in zip(mod.parameters(), want[i][1]):
            assert torch.equal(p.grad, g)
    with pytest.raises(RuntimeError, match='second backward'):
        outs[0].backward(cots[0])
    with torch.no_grad():
        assert torch.equal(_node(mod, xs[2]), _node(mod, xs[2].clone().requires_grad_(True)).detach())


def _modules_match_fp64(mod, ref, x, call):
    """what the node refuses ran the modules and still matches fp64"""
    xg = x.cuda().requires_grad_(True)
    out = call(mod, xg)
    assert type(out.grad_fn).__name__ != NODE
    xr = x.double().requires_grad_(True)
    out_ref = K.modules_forward(ref, xr)
    cot = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(9))
    for p in list(mod.parameters()) + list(ref.parameters()):
        p.grad = None
    out.backward(cot.cuda())
    out_ref.backward(cot.double())
    assert float((out.detach().cpu().double() - out_ref.detach()).abs().max() / out_ref.detach().abs().max()) <= 1e-4
    assert float((xg.grad.cpu().double() - xr.grad).norm() / xr.grad.norm()) <= 1e-3
    for (name, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters()):
        assert float((p.grad.cpu().double() - q.grad).norm() / q.grad.norm()) <= 1e-3, name


def test_what_the_node_refuses_runs_the_modules():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import downconv
    case = ('down', 2, 64, 64, 8)
    mod, ref = K.module_pair(case, 1)
    mod = mod.cuda()
    x = K.case_inputs(case, 1)[0]
    assert type(_node(mod, x.cuda()).grad_fn).__name__ == NODE
    # a tracked BatchNorm2d (training mode: the batch's statistics, as the fp64 copy's)
    tracked, tracked_ref = K.module_pair(case, 1)
    tracked[0], tracked_ref[0] = nn.BatchNorm2d(64), nn.BatchNorm2d(64).double()
    assert not downconv.bn_fusable(x.cuda(), tracked.cuda()[0], tracked[2])
    _modules_match_fp64(tracked, tracked_ref, x, _node)
    # 96 channels, a 3 x 3 convolution, a hook on the norm, a GroupNorm
    m96, r96 = K.module_pair(('down', 2, 96, 96, 8), 1)
    _modules_match_fp64(m96.cuda(), r96, torch.randn(2, 96, 8, 8, generator=torch.Generator().manual_seed(3)), _node)
    other, other_ref = K.module_pair(case, 1)
    other[2] = nn.Conv2d(64, 64, 3, 2, 1)
    other_ref[2] = nn.Conv2d(64, 64, 3, 2, 1).double()
    other_ref[2].load_state_dict(other[2].state_dict())
    _modules_match_fp64(other.cuda(), other_ref, x, _node)
    handle = mod[0].register_forward_hook(lambda m, i, o: None)
    assert not downconv.bn_fusable(x.cuda(), mod[0], mod[2])
    _modules_match_fp64(mod, ref, x, _node)
    handle.remove()
    assert downconv.bn_fusable(x.cuda(), mod[0], mod[2]) and not downconv.fusable(x.cuda(), mod[0], mod[2])
    # slices > 1 with a backward to come: refused by bn_fusable; the library says why when asked directly
    assert not downconv.bn_fusable(x.cuda(), mod[0], mod[2], slices=2)
    with torch.no_grad():
        assert downconv.bn_fusable(x.cuda(), mod[0], mod[2], slices=2) and not downconv.bn_fusable(x.cuda(), mod[0], mod[2], slices=3)
    with pytest.raises(nof._lib.NodeHipUnsupported, match='keep_for_backward = 0 only'):
        downconv._BnDownConvFn.apply(x.cuda(), 1e-5, True, 2, *[p.detach() for p in mod.parameters()])
    # gn_relu_conv and a GroupNorm hand-off take the paths they took
    gn = nn.GroupNorm(32, 64).cuda()
    assert type(downconv.gn_relu_conv(x.cuda(), gn, mod[2]).grad_fn).__name__ == '_DownConvFnBackward'


def test_no_miopen_or_aten_norm_kernel_in_a_fused_step():
    from torch.profiler import ProfilerActivity, profile
    case = ('down', 2, 64, 64, 8)
    mod = K.module_pair(case, 1)[0].cuda()
    x = K.case_inputs(case, 1)[0].cuda().requires_grad_(True)
    _node(mod, x).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = _node(mod, x)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('miopen', 'batch_norm', 'igemm', 'batched_transpose'))]
    assert not bad, bad
    assert any('_BnDownConvFn' in k for k in names), names


# ---------------------------------------------------------------------------------------------------------------------
# the sliced call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,mode', [r for case in K.SLICED_CASES for r in K.runs(case)], ids=_id)
def test_every_slice_of_the_sliced_call_is_its_own_unsliced_call_bit_for_bit(case, mode):
    """... and within the bound of the fp64 per-slice modules; the flattened T N batch with slices = 1 (statistics over all slices)
    differs from both, so the slices of this input do not happen to share their statistics."""
    seed = K.seed_of(case, mode)
    mod, ref = K.module_pair(case, seed, mode)
    mod = mod.cuda()
    x, _ = K.case_inputs(case, seed)
    t, n = x.shape[:2]
    xc = x.cuda()
    flat = xc.reshape(t * n, *x.shape[2:])
    with torch.no_grad():
        sliced = _node(mod, flat, t)
        assert sliced.grad_fn is None and sliced.shape[0] == t * n
        sliced = sliced.reshape(t, n, *sliced.shape[1:])
        alone = torch.stack([_node(mod, xi) for xi in xc])
        together = _node(mod, flat).reshape(sliced.shape)
        want64 = K.modules_forward(ref, x.double())
        want32 = K.modules_forward(mod.cpu(), x)
    for i in range(t):
        assert torch.equal(sliced[i], alone[i]), i
    assert torch.equal(_node(mod.cuda(), flat.clone().requires_grad_(True)).detach().reshape(sliced.shape), together)      # (the keeping forward too)
    scale = float(want64.abs().max())
    err = float((sliced.cpu().double() - want64).abs().max()) / scale
    floor = float((want32.double() - want64).abs().max()) / scale
    off = float((together.cpu().double() - want64).abs().max()) / scale
    print('bndownconv sliced %s %s: output max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e; the flattened batch: %.2e)'
          % (_id(case), mode, err, floor, K.bound(floor), off))
    assert err <= K.bound(floor)
    assert off > 100 * K.bound(floor) and not torch.equal(together, sliced)


class _Trajectory(nn.Module):
    """stands in for the ODE block: T fixed affine images of its input, so the statistics of the slices differ and the trajectory is
    the same bits with and without gradients (no solve: the hand-off is what is tested)"""

    def __init__(self, t):
        super().__init__()
        self.t = t
        self.return_last_only = False

    def forward(self, x):
        return torch.stack([x * (1.0 + 0.5 * k) + 0.1 * k for k in range(self.t)])


def _ode2(mode='kinkfree'):
    import neural_ode_features_amd as nof
    torch.manual_seed(K.KINK_FREE_SEED)
    ds = nof.ODEDownsample2(3, 64, adjoint=True, t1=[0.5, 1.0], norm='batch')
    assert ds.odeblock.integration_time.tolist() == [0.0, 0.5, 1.0]         # a three-point t1
    with torch.no_grad():
        ds.norm[0].weight.add_(0.2 * torch.randn(64))
        ds.norm[0].bias.add_(0.2 * torch.randn(64) + 8.0)                    # kink-free: no ReLU mask can differ
    return ds


def test_ode2_trajectory_is_one_sliced_call_without_gradients_and_t_calls_with():
    import copy
    from neural_ode_features_amd import downconv
    ds = _ode2()
    ds.odeblock = _Trajectory(3)
    ds = ds.cuda()
    ds.apply_conv = True
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1)).cuda()
    fn = downconv._BnDownConvFn
    with torch.no_grad(), mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        traj, cont = ds(x)
    assert node.call_count == 1 and node.call_args[0][3] == 3              # ONE call, three slices
    assert traj.shape == (3, 2, 64, 4, 4) and torch.equal(cont, traj[-1]) and torch.isfinite(traj).all()
    try:
        ds.fused_handoff = False
        with torch.no_grad(), mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
            mods, _ = ds(x)
        assert node.call_count == 0
    finally:
        del ds.fused_handoff
    assert float((traj - mods).abs().max() / mods.abs().max()) <= 1e-4       # (two fp32 paths: the refusal tests' bound)
    # apply_conv off: per-slice norms, the last slice through the unsliced node
    ds.apply_conv = False
    with torch.no_grad(), mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        normed, cont2 = ds(x)
    assert node.call_count == 1 and node.call_args[0][3] == 1 and normed.shape == (3, 2, 64, 8, 8)
    assert torch.equal(cont2, cont)
    ds.apply_conv = True
    # with a backward possible: T unsliced calls, autograd sums the shared parameters' gradients.  Everything in front of the
    # hand-off is frozen, so its four gradients are the whole backward; the reference runs the fp64 modules slice by slice on
    # the trajectory the hand-off was given
    for p in ds.conv1.parameters():
        p.requires_grad_(False)
    seen = []
    hook = ds.odeblock.register_forward_hook(lambda m, i, o: seen.append(o.detach().clone()))
    with mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        traj_g, _ = ds(x)
    hook.remove()
    assert node.call_count == 3 and all(c[0][3] == 1 for c in node.call_args_list)
    assert torch.equal(traj_g.detach(), traj)                                # every slice the bits of the sliced call's
    cot = torch.randn(traj.shape, generator=torch.Generator().manual_seed(2))
    traj_g.backward(cot.cuda())
    got = {k: p.grad.cpu() for k, p in (('0.weight', ds.norm[0].weight), ('0.bias', ds.norm[0].bias), ('2.weight', ds.conv2.weight), ('2.bias', ds.conv2.bias))}
    states = seen[0].cpu()
    assert states.shape == (3, 2, 64, 8, 8)
    mod32 = nn.Sequential(copy.deepcopy(ds.norm[0]).cpu(), nn.ReLU(), copy.deepcopy(ds.conv2).cpu())
    mod64 = copy.deepcopy(mod32).double()
    r64 = K.run_modules(mod64, states.double(), cot.double())
    r32 = K.run_modules(mod32, states, cot)
    errs = T.errors((traj_g.detach(), r32[1], got, ()), r64)
    floor = T.errors(r32, r64)
    for k in ('output', 'grad 0.weight', 'grad 0.bias', 'grad 2.weight', 'grad 2.bias'):
        print('ode2 trajectory with gradients: %-14s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (k, errs[k], floor[k], K.bound(floor[k])))
        assert errs[k] <= K.bound(floor[k]), k


def test_ode2_solves_a_real_trajectory_through_one_sliced_call():
    """the stem as `evaluate accuracy` sets it up: a dense-output solve of the `norm='batch'` dynamics, then ONE node call"""
    from neural_ode_features_amd import downconv
    ds = _ode2().cuda().eval()
    ds.odeblock.tol = 1e-2
    ds.odeblock.return_last_only = False
    ds.apply_conv = True
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1)).cuda()
    fn = downconv._BnDownConvFn
    with torch.no_grad(), mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        traj, cont = ds(x)
    assert node.call_count == 1 and node.call_args[0][3] == 3
    assert traj.shape == (3, 2, 64, 4, 4) and torch.isfinite(traj).all() and torch.equal(cont, traj[-1])


def test_command_lines_train_and_features(tmp_path):
    """`train --norm batch -d ode2 -a -t 1e-2` (one epoch, synthetic data), then `evaluate features`: the hand-off is the node in
    both, every output finite."""
    import numpy as np
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as Tr
    run = str(tmp_path / 'run')
    fn = nof.downconv._BnDownConvFn
    with mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        assert Tr.main(['--norm', 'batch', '-d', 'ode2', '-f', '64', '--dataset', 'mnist', '--synthetic-size', '64', '-b', '32', '-e', '1', '-a',
                        '-t', '1e-2', '--run-dir', run]) == 0
    assert node.call_count >= 2                          # one per batch
    ckpt = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ckpt['params']['norm'] == 'batch' and ckpt['params']['downsample'] == 'ode2' and math.isfinite(ckpt['metrics']['loss'])
    with mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        E.main(['features', run])
    assert node.call_count >= 1
    with np.load(os.path.join(run, 'features.npz')) as f:
        assert np.isfinite(f['features']).all() and f['features'].shape[-1] == 64

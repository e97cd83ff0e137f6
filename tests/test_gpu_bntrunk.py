"""GPU: the `norm='batch'` residual trunk as one HIP node (resnet.py `_BnTrunkFn`, csrc/bntrunk_api.hip: node_bntrunk_fwd /
node_bntrunk_bwd; reference model.py:79, :284-310 with model.py:274) and the whole `ResNet(..., norm='batch')` on it.

Reference: the same modules as `.double()` on the CPU (tests/bntrunk_cases.py), never the node.  Metric: max-norm error over max|ref|
for the output, the input gradient and every tap; parameter gradients relative to max(max|ref|, 1e-4 x the largest gradient).  Bound
per quantity: max(2e-5 max(1, blocks / 2), 4 x the same error of the fp32 modules on the CPU), computed here -- the first term is
tests/test_gpu_resnet.py::bound, the second tests/test_gpu_bnfunc.py's allowance for two correct fp32 summation orders.

Every run asserts `type(out.grad_fn).__name__ == '_BnTrunkFnBackward'`: without the node the module sequence runs and every test
built on `run_node` fails.

Worst measured error per case on an MI355X (ordinary / kinkfree / split; the quantity is a norm's weight or bias gradient everywhere but
where named; bounds 2e-5 at one or two blocks, 6e-5 at six):
    (64, 8, 2, 1)        9.1e-7 / 1.9e-6 / 2.8e-6        (64, 16, 1, 2)       9.2e-7 / 3.1e-6 / 4.0e-6
    (64, 7, 3, 2)        8.1e-7 / 1.9e-6 / 1.3e-6        (64, (6, 5), 1, 1)   6.4e-7 (conv1 weight) / 1.4e-6 / 1.4e-6
    (128, 8, 2, 6)       1.5e-6 / 3.0e-6 / 2.5e-6        (64, 7, 84, 2)       1.8e-6 / 5.5e-6 / 4.1e-6
    (256, 8, 2, 6)       2.7e-6 / 4.5e-6 / 4.6e-6        (256, 8, 33, 2)      (no admissible seed) / 8.0e-6 / 7.8e-6
    (192, 8, 2, 2)       1.5e-6 / 3.8e-6 / 3.1e-6        (64, 8, 5, 2)        7.6e-7 / 2.6e-6 / 2.2e-6
    (64, 1, 4, 1)        2.1e-6 (conv1 weight) / 7.1e-5 / 1.6e-4, both grad norm1.bias, where the fp32 modules on the CPU stand at 4.2e-5 and
                         8.9e-5 (bounds 1.7e-4 and 3.5e-4 by the second term): four values per channel, biases of 8 behind variances of O(1)
Whole model (kink-free / split; no ordinary seed is admissible, bntrunk_cases.py): worst 5.4e-5 / 5.9e-5, the one-shot stem's bias gradient, which is
zero identically in front of a BatchNorm (the fp32 modules on the CPU: 5.4e-5 / 6.8e-5); logits 2.4e-7, features against the module path 2.2e-7."""
import copy
import math
import os

import pytest
import torch

from tests import bnfunc_cases as B
from tests import bntrunk_cases as T

pytestmark = pytest.mark.gpu
NODE = '_BnTrunkFnBackward'


def _id(v):
    if isinstance(v, str):
        return v
    c, side, n, blocks = v
    return 'c%d_%s_n%d_b%d' % (c, '%dx%d' % side if isinstance(side, tuple) else side, n, blocks)


def run_node(case, mode, trunk=None):
    """Forward (with taps) + backward of the node on the GPU: (out, d_x, parameter gradients by name, taps)."""
    seed = T.seed_of(case, mode)
    if trunk is None:
        trunk = T.trunk_pair(case, seed, mode)[0]
    trunk = trunk.cuda()
    x, cot = T.case_inputs(case, seed)
    xg = x.cuda().requires_grad_(True)
    out, taps = trunk.forward_taps(xg)
    assert type(out.grad_fn).__name__ == NODE          # the node, not the module sequence
    assert torch.equal(taps[-1], out)
    out.backward(cot.cuda())
    return out.detach(), xg.grad, {k: p.grad for k, p in trunk.named_parameters()}, taps


RUNS = [r for case in T.ALL_CASES for r in T.runs(case)]


@pytest.mark.parametrize('case,mode', RUNS, ids=_id)
def test_output_taps_and_every_gradient_match_fp64(case, mode):
    r64, r32 = T.references(case, mode)
    errs, floor = T.errors(run_node(case, mode), r64), T.errors(r32, r64)
    bad = {}
    for k, v in errs.items():
        bnd = T.bound(case[3], floor[k])
        print('bntrunk %s %s: %-32s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (_id(case), mode, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    worst = max(errs, key=errs.get)
    print('bntrunk %s %s: WORST %s %.2e' % (_id(case), mode, worst, errs[worst]))
    assert not bad, bad


@pytest.mark.parametrize('blocks', [1, 3])
def test_shortcut_gradient_is_the_cotangent_bit_for_bit(blocks):
    """Convolution weights at zero: every block is the identity, its norm1 backward pass receives a zero gradient, and what it
    writes is 0 + the shortcut's gradient -- the `skip` variant of k_bn_bwd_dx alone."""
    case = (64, 7, 3, blocks)
    trunk = T.trunk_pair(case, 3)[0]
    with torch.no_grad():
        for blk in trunk:
            blk.conv1.weight.zero_()
            blk.conv2.weight.zero_()
    trunk = trunk.cuda()
    x, cot = T.case_inputs(case, 3)
    xg = x.cuda().requires_grad_(True)
    out = trunk(xg)
    assert type(out.grad_fn).__name__ == NODE
    assert torch.equal(out, xg.detach())
    out.backward(cot.cuda())
    assert torch.equal(xg.grad.cpu(), cot)
    for name, p in trunk.named_parameters():
        if 'norm1' in name or 'conv1' in name:       # nothing reaches the first half of a block
            assert not p.grad.any(), name


def test_two_runs_return_the_same_bits():
    case, mode = (64, 7, 84, 2), 'ordinary'
    a, b = run_node(case, mode), run_node(case, mode)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for u, v in zip(a[3], b[3]):
        assert torch.equal(u, v)


def test_forwards_in_flight_keep_their_own_workspaces():
    case = (64, 7, 3, 2)
    trunk = T.trunk_pair(case, 8)[0].cuda()
    xs = [T.case_inputs(case, s)[0].cuda() for s in (1, 2, 3)]
    cots = [T.case_inputs(case, s)[1].cuda() for s in (1, 2)]

    def alone(i):
        for p in trunk.parameters():
            p.grad = None
        x = xs[i].clone().requires_grad_(True)
        trunk(x).backward(cots[i])
        return x.grad, [p.grad.clone() for p in trunk.parameters()]
    want = [alone(0), alone(1)]
    for order in ((0, 1), (1, 0)):
        ins = [xs[i].clone().requires_grad_(True) for i in (0, 1)]
        outs = [trunk(ins[0])]
        with torch.no_grad():
            free = trunk(xs[2])
        outs.append(trunk(ins[1]))
        assert all(type(o.grad_fn).__name__ == NODE for o in outs) and free.grad_fn is None
        for i in order:
            for p in trunk.parameters():
                p.grad = None
            outs[i].backward(cots[i], retain_graph=True)
            assert torch.equal(ins[i].grad, want[i][0])
            for p, g in zip(trunk.parameters(), want[i][1]):
                assert torch.equal(p.grad, g)
        with pytest.raises(RuntimeError, match='second backward'):
            outs[0].backward(cots[0])


def test_what_the_node_refuses_runs_the_module_sequence():
    import neural_ode_features_amd as nof
    case = (64, 8, 2, 2)
    x = T.case_inputs(case, 1)[0].cuda().requires_grad_(True)
    trunk = T.trunk_pair(case, 1)[0].cuda()
    assert type(trunk(x).grad_fn).__name__ == NODE
    trunk.fused_batch = False
    assert type(trunk(x).grad_fn).__name__ != NODE
    del trunk.fused_batch
    try:
        nof.resnet.ResidualTrunk.fused_batch = False
        assert type(trunk(x).grad_fn).__name__ != NODE
    finally:
        nof.resnet.ResidualTrunk.fused_batch = True
    assert type(trunk(x).grad_fn).__name__ == NODE
    tracked = copy.deepcopy(trunk)
    tracked[1].norm1 = torch.nn.BatchNorm2d(64).cuda()
    assert type(tracked(x).grad_fn).__name__ != NODE
    c96 = nof.resnet.ResidualTrunk(96, 2, norm='batch').cuda()
    out = c96(torch.randn(2, 96, 8, 8, device='cuda', requires_grad=True))
    assert type(out.grad_fn).__name__ != NODE
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):      # N H W = 1: what nn.BatchNorm2d raises
        trunk(torch.randn(1, 64, 1, 1, device='cuda'))
    # the GroupNorm trunk takes the path it took
    gn = nof.resnet.ResidualTrunk(64, 2).cuda()
    assert type(gn(x).grad_fn).__name__ == '_TrunkFnBackward'


def test_no_miopen_or_aten_norm_kernel_in_a_fused_step():
    from torch.profiler import ProfilerActivity, profile
    case = (64, 8, 2, 2)
    trunk = T.trunk_pair(case, 1)[0].cuda()
    x = T.case_inputs(case, 1)[0].cuda().requires_grad_(True)
    trunk(x).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = trunk(x)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('miopen', 'batch_norm', 'igemm', 'batched_transpose'))]
    assert not bad, bad
    assert any('_BnTrunkFn' in k for k in names), names


def test_batch_norm_dynamics_still_return_the_same_bits_run_to_run():
    """The dx pass gained a compile-time variant; the two instances the dynamics launch are what they were.  Their values are
    tests/test_gpu_bnfunc.py's to check (unchanged); here: one forward + backward at (5, 64, 8, 8), twice, identical bits."""
    case, seed = (5, 64, 8, 8), B.MULTI_SEEDS[(5, 64, 8, 8)]

    def run():
        func = B.func_pair(64, seed)[0].cuda()
        x, cot = B.case_inputs(case, seed)
        xg = x.cuda().requires_grad_(True)
        tg = torch.tensor(B.T_EVAL, device='cuda').requires_grad_(True)
        out = func(tg, xg)
        assert type(out.grad_fn).__name__ == '_BatchOdeFnBackward'
        out.backward(cot.cuda())
        return [out.detach(), xg.grad, tg.grad] + [p.grad for p in func.parameters()]
    for u, v in zip(run(), run()):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', T.MODEL_MODES)
def test_whole_model_logits_and_every_gradient_match_fp64(mode):
    """ResNet(3, 64 filters, one-shot stem, norm='batch') at [4, 3, 32, 32]: stem, trunk node, BatchNorm head node, Linear.  (No
    seed is admissible for ordinary parameters at this size: bntrunk_cases.py.)"""
    net = T.model_pair(T.KINK_FREE_SEED, mode)[0].cuda()
    x, cot = T.model_inputs(T.KINK_FREE_SEED)
    seen = []
    hooks = [net.features.register_forward_hook(lambda m, i, o: seen.append(type(o.grad_fn).__name__))]
    got = T.run_model(net, x.cuda(), cot.cuda())
    hooks[0].remove()
    assert seen == [NODE]
    r64, r32, _, _ = T.model_references(mode)
    errs, floor = T.model_errors(got, r64), T.model_errors(r32, r64)
    bad = {}
    for k, v in errs.items():
        bnd = T.bound(6, floor[k])
        print('bn resnet %s: %-40s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (mode, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    assert not bad, bad


@pytest.mark.parametrize('mode', T.MODEL_MODES)
def test_features_extractor_reads_seven_time_points_from_one_forward(mode):
    import neural_ode_features_amd as nof
    from unittest import mock
    net = T.model_pair(T.KINK_FREE_SEED, mode)[0].cuda().eval()
    net.to_features_extractor()
    x = T.model_inputs(T.KINK_FREE_SEED)[0].cuda()
    with torch.no_grad(), mock.patch.object(nof.resnet._BnTrunkFn, 'apply', wraps=nof.resnet._BnTrunkFn.apply) as node:
        fused = net(x)
    assert node.call_count == 1 and fused.shape == (7, 4, 64)
    try:
        nof.resnet.ResidualTrunk.fused_batch = nof.FCClassifier.fused_batch = False
        with torch.no_grad():
            mods = net(x)
    finally:
        nof.resnet.ResidualTrunk.fused_batch = nof.FCClassifier.fused_batch = True
    _, _, f64, f32 = T.model_references(mode)
    scale = float(f64.abs().max())
    floor = float((f32.double() - f64).abs().max()) / scale
    bnd = T.bound(6, floor)
    err = float((fused.double() - mods.double()).abs().max()) / scale
    err64 = float((fused.cpu().double() - f64).abs().max()) / scale
    print('bn resnet %s features: fused against the module path %.2e, against fp64 %.2e (fp32 modules on the CPU %.2e, bound %.1e)' % (mode, err, err64, floor, bnd))
    assert err <= bnd and err64 <= bnd


def test_command_lines_train_and_features(tmp_path):
    """`train --model resnet --norm batch` (one epoch, synthetic data), then `evaluate features` on the run."""
    import numpy as np
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as Tr
    run = str(tmp_path / 'run')
    assert Tr.main(['--model', 'resnet', '--norm', 'batch', '-f', '64', '-d', 'one-shot', '--synthetic-size', '64', '-b', '32', '-e', '1',
                    '--run-dir', run]) == 0
    ckpt = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ckpt['params']['norm'] == 'batch' and ckpt['params']['model'] == 'resnet'
    assert math.isfinite(ckpt['metrics']['loss'])
    assert 'features.5.norm2.weight' in ckpt['model'] and not any('running_mean' in k for k in ckpt['model'])
    E.main(['features', run])
    with np.load(os.path.join(run, 'features.npz')) as f:
        assert f['features'].shape[1] == 7 and f['features'].shape[-1] == 64
        assert np.isfinite(f['features']).all()

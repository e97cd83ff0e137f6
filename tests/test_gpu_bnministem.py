"""GPU: the `norm='batch'` minimal stem as one HIP node (ministem.py `_BnMiniStemFn`, csrc/bnministem_api.hip: node_bnministem_fwd /
node_bnministem_bwd; reference model.py:129-145 with model.py:274), the whole `ResNet(..., downsample='minimal', norm='batch')` on it
and the command lines that pick it up.

Reference: the same modules as `.double()` on the CPU (tests/bnministem_cases.py), never the node.  Metric: bntrunk_cases.errors --
max-norm error over max|ref| for the output and the image gradient; parameter gradients relative to max(max|ref|, 1e-4 x the
largest gradient) (the gradients of the first two convolutions' biases are zero identically in front of a BatchNorm).  Bound per
quantity: max(2e-5, 4 x the same error of the fp32 modules on the CPU), computed here -- tests/bnstem_cases.py's, unchanged.

Every run sets `stem.fused_batch = True` and asserts `type(out.grad_fn).__name__ == '_BnMiniStemFnBackward'`: without the node the
module sequence runs and every test here fails.

Worst measured error per case on an MI355X (ordinary / kinkfree / split), the two zero bias gradients apart; bound 2e-5 where no
other is given:
    (1, 28, 64, 2)       5.6e-7 (the last convolution's weight gradient) / 1.6e-6 (the first norm's bias gradient) / 1.1e-6 (the
                         middle convolution's weight gradient)
    (3, 32, 128, 3)      6.5e-7 (image gradient) / 2.6e-6 / 3.2e-6 (the first norm's bias gradient)
    (3, 32, 256, 2)      9.1e-7 (the second norm's weight gradient) / 1.2e-6 / 3.6e-6 (the first norm's bias gradient)
    (3, (12, 10), 64, 2) 7.4e-7 (image gradient) / 1.3e-6 / 1.1e-6 (the first norm's bias gradient)
    (1, 10, 64, 1)       7.1e-7 (the middle convolution's weight gradient) / 7.0e-7 / 8.7e-7 (the first norm's bias gradient)
    (3, 32, 64, 5)       5.0e-7 (output) / 1.6e-6 / 2.4e-6 (the first norm's bias gradient)
Output at most 1.1e-6, image gradient at most 7.7e-7.  The bias gradients of the first two convolutions are zero identically in
front of a BatchNorm; relative to 1e-4 x the largest gradient they stand at 2.5e-5 .. 2.7e-3 (worst: (3, 32, 64, 5) ordinary), where
the fp32 modules on the CPU stand at 1.8e-5 .. 3.8e-3; always inside 4 x the latter (closest: 3.bias of (3, (12, 10), 64, 2) split,
1.9e-4 against a bound of 3.0e-4).
Whole model (kink-free / split): worst 6.4e-5 / 5.1e-5, conv1 weight gradients of trunk blocks 5 and 2 (the fp32 modules on the
CPU: 6.8e-5 / 4.8e-5 there; bound 4 x those, 2.7e-4 / 1.9e-4)."""
import math
import os

import pytest
import torch

from tests import bnministem_cases as K

pytestmark = pytest.mark.gpu
NODE = '_BnMiniStemFnBackward'
ZERO_GRADS = ('grad 0.bias', 'grad 3.bias')


def _id(v):
    if isinstance(v, str):
        return v
    return '_'.join('%dx%d' % s if isinstance(s, tuple) else str(s) for s in v)


def run_node(case, mode, stem=None, frozen=False):
    """Forward + backward of the node on the GPU with `input_grad` on: (out, d_x, parameter gradients by name, ())."""
    seed = K.seed_of(case, mode)
    if stem is None:
        stem = K.module_pair(case, seed, mode)[0]
    stem = stem.cuda()
    stem.fused_batch = True
    stem.input_grad = True
    if frozen:
        for p in stem.parameters():
            p.requires_grad_(False)
    x, cot = K.case_inputs(case, seed)
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == NODE          # the node, not the module sequence
    out.backward(cot.cuda())
    return out.detach(), xg.grad, {k: p.grad for k, p in stem.named_parameters()}, ()


def check_against_fp64(case, mode, got, tag=''):
    r64, r32 = K.references(case, mode)
    errs, floor = K.errors(got, r64), K.errors(r32, r64)
    assert len(errs) == 2 + 10
    bad = {}
    for k, v in errs.items():
        bnd = K.bound(floor[k])
        print('bnministem %s %s%s: %-16s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (_id(case), mode, tag, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    rest = {k: v for k, v in errs.items() if k not in ZERO_GRADS}
    worst = max(rest, key=rest.get)
    print('bnministem %s %s%s: WORST %s %.2e' % (_id(case), mode, tag, worst, rest[worst]))
    assert not bad, bad


RUNS = [r for case in K.ALL_CASES for r in K.runs(case)]


@pytest.mark.parametrize('case,mode', RUNS, ids=_id)
def test_output_image_gradient_and_every_parameter_gradient_match_fp64(case, mode):
    check_against_fp64(case, mode, run_node(case, mode))


def test_the_cases_reach_their_regimes():
    reached = set()
    for case, asked in K.MULTI.items():
        plan = K.plan_of(case)
        for norm, regime in asked:
            assert K.REGIMES[regime](plan[norm]), (case, norm, regime, plan[norm])
            reached.add(regime)
    assert reached == set(K.REGIMES)
    assert all(case in K.ALL_CASES for case in K.MULTI)


def test_frozen_parameters_leave_the_image_gradient_bit_for_bit():
    """grads = NULL: the data-gradient chain alone.  d_x has the bits of the run with parameter gradients; no parameter has a .grad."""
    case, mode = (3, 32, 64, 5), 'ordinary'
    full, frozen = run_node(case, mode), run_node(case, mode, frozen=True)
    assert torch.equal(full[0], frozen[0])
    assert torch.equal(full[1], frozen[1])
    assert all(g is None for g in frozen[2].values()) and all(g is not None for g in full[2].values())


def test_parameter_gradients_are_the_same_bits_with_and_without_the_image_gradient():
    """d_x = NULL (input_grad off, an input that requires none) against the full backward"""
    case, mode = (3, 32, 64, 5), 'ordinary'
    seed = K.seed_of(case, mode)
    stem = K.module_pair(case, seed, mode)[0].cuda()
    stem.fused_batch = True
    x, cot = K.case_inputs(case, seed)
    out = stem(x.cuda())
    assert type(out.grad_fn).__name__ == NODE
    out.backward(cot.cuda())
    with_dx = run_node(case, mode)
    assert torch.equal(out.detach(), with_dx[0])
    for k, p in stem.named_parameters():
        assert torch.equal(p.grad, with_dx[2][k]), k


def test_two_runs_return_the_same_bits():
    case, mode = (3, 32, 64, 5), 'kinkfree'
    a, b = run_node(case, mode), run_node(case, mode)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_forwards_in_flight_keep_their_own_workspaces():
    case = (1, 28, 64, 2)
    stem = K.module_pair(case, 5)[0].cuda()
    stem.fused_batch = True
    stem.input_grad = True
    xs = [K.case_inputs(case, s)[0].cuda() for s in (1, 2, 3)]
    cots = [K.case_inputs(case, s)[1].cuda() for s in (1, 2)]

    def alone(i):
        for p in stem.parameters():
            p.grad = None
        x = xs[i].clone().requires_grad_(True)
        stem(x).backward(cots[i])
        return x.grad, [p.grad.clone() for p in stem.parameters()]
    want = [alone(0), alone(1)]
    for order in ((0, 1), (1, 0)):
        ins = [xs[i].clone().requires_grad_(True) for i in (0, 1)]
        outs = [stem(ins[0])]
        with torch.no_grad():
            free = stem(xs[2])
        outs.append(stem(ins[1]))
        assert all(type(o.grad_fn).__name__ == NODE for o in outs) and free.grad_fn is None
        for i in order:
            for p in stem.parameters():
                p.grad = None
            outs[i].backward(cots[i], retain_graph=True)
            assert torch.equal(ins[i].grad, want[i][0])
            for p, g in zip(stem.parameters(), want[i][1]):
                assert torch.equal(p.grad, g)
        with pytest.raises(RuntimeError, match='second backward'):
            outs[0].backward(cots[0])
    # the no-grad forward (the stream's scratch) returns the bits of the forward that keeps everything
    with torch.no_grad():
        assert torch.equal(stem(xs[2]), stem(xs[2].clone().requires_grad_(True)).detach())


def _modules_match_fp64(stem, ref, x, requires_grad=False):
    """a refused stem ran the module sequence and still matches fp64 (the bounds of test_gpu_bnconvstem.py's refusal test)"""
    xg = x.cuda().requires_grad_(requires_grad)
    out = stem(xg)
    assert type(out.grad_fn).__name__ not in (NODE, '_MiniStemFnBackward')
    out_ref = ref(x.double())
    cot = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(9))
    for p in list(stem.parameters()) + list(ref.parameters()):
        p.grad = None
    out.backward(cot.cuda())
    out_ref.backward(cot.double())
    assert float((out.detach().cpu().double() - out_ref.detach()).abs().max() / out_ref.detach().abs().max()) <= 1e-4
    for (name, p), (_, q) in zip(stem.named_parameters(), ref.named_parameters()):
        if name in ('0.bias', '3.bias') and isinstance(ref[1], torch.nn.BatchNorm2d):         # zero identically in front of a BatchNorm: nothing to be relative to
            continue
        assert float((p.grad.cpu().double() - q.grad).norm() / q.grad.norm()) <= 1e-3, name


def test_what_the_node_refuses_runs_the_module_sequence():
    import neural_ode_features_amd as nof
    case = (3, 32, 64, 2)
    stem, ref = K.module_pair(case, 1)
    stem = stem.cuda()
    x = K.case_inputs(case, 1)[0]
    stem.fused_batch = True
    assert type(stem(x.cuda()).grad_fn).__name__ == NODE
    stem.fused_batch = False
    _modules_match_fp64(stem, ref, x)
    del stem.fused_batch
    default = nof.ministem.MinimalStem.fused_batch
    try:
        nof.ministem.MinimalStem.fused_batch = False
        _modules_match_fp64(stem, ref, x)
    finally:
        nof.ministem.MinimalStem.fused_batch = default
    stem.fused_batch = True
    assert type(stem(x.cuda()).grad_fn).__name__ == NODE
    # an input that requires a gradient, input_grad off
    assert stem.input_grad is False
    _modules_match_fp64(stem, ref, x, requires_grad=True)
    # a tracked BatchNorm2d in one slot (training mode: it normalises with the batch's statistics, as the fp64 copy does)
    tracked, tracked_ref = K.module_pair(case, 1)
    tracked[4] = torch.nn.BatchNorm2d(24)
    tracked_ref[4] = torch.nn.BatchNorm2d(24).double()
    tracked.fused_batch = True
    _modules_match_fp64(tracked.cuda(), tracked_ref, x)
    # filters = 96
    s96, r96 = K.module_pair((3, 32, 96, 2), 1)
    s96.fused_batch = True
    _modules_match_fp64(s96.cuda(), r96, x)
    # the GroupNorm stem at the same shape takes the path it took
    gn = nof.ODENet(3, out=10, n_filters=64, downsample='minimal', adjoint=True).downsample.module.cuda()
    assert type(gn(x.cuda()).grad_fn).__name__ == '_MiniStemFnBackward'


def test_no_miopen_or_aten_norm_kernel_in_a_fused_step():
    from torch.profiler import ProfilerActivity, profile
    case = (3, 32, 64, 2)
    stem = K.module_pair(case, 1)[0].cuda()
    stem.fused_batch = True
    stem.input_grad = True
    x = K.case_inputs(case, 1)[0].cuda().requires_grad_(True)
    stem(x).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = stem(x)
        assert type(out.grad_fn).__name__ == NODE
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('miopen', 'batch_norm', 'igemm', 'batched_transpose'))]
    assert not bad, bad
    assert any('_BnMiniStemFn' in k for k in names), names
    assert any('k_bnmini_' in k for k in names), names


# ---------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', K.MODEL_MODES)
def test_whole_model_logits_and_every_gradient_match_fp64(mode):
    """ResNet(3, 64 filters, minimal stem, norm='batch') at [4, 3, 32, 32]: stem node, trunk node, BatchNorm head node, Linear."""
    net = K.model_pair(K.KINK_FREE_SEED, mode)[0].cuda()
    net.downsample.module.fused_batch = True
    for m in net.modules():
        if hasattr(m, 'input_grad'):
            m.input_grad = True            # (run_model asks for the image's gradient)
    x, cot = K.model_inputs(K.KINK_FREE_SEED)
    seen = []
    hooks = [net.downsample.module.register_forward_hook(lambda m, i, o: seen.append(type(o.grad_fn).__name__)),
             net.features.register_forward_hook(lambda m, i, o: seen.append(type(o.grad_fn).__name__))]
    got = K.run_model(net, x.cuda(), cot.cuda())
    for h in hooks:
        h.remove()
    assert seen == [NODE, '_BnTrunkFnBackward']
    r64, r32 = K.model_references(mode)
    errs, floor = K.model_errors(got, r64), K.model_errors(r32, r64)
    bad = {}
    for k, v in errs.items():
        bnd = K.model_bound(K.MODEL_BLOCKS, floor[k])
        print('bn resnet (minimal stem) %s: %-40s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (mode, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    worst = max(errs, key=errs.get)
    print('bn resnet (minimal stem) %s: WORST %s %.2e' % (mode, worst, errs[worst]))
    assert not bad, bad


def _mnist_blob(path):
    gen = torch.Generator().manual_seed(5)
    blob = dict(x_train=torch.randint(0, 256, (64, 1, 28, 28), generator=gen).to(torch.uint8), y_train=torch.arange(64) % 10,
                x_test=torch.randint(0, 256, (32, 1, 28, 28), generator=gen).to(torch.uint8), y_test=torch.zeros(32, dtype=torch.int64))
    torch.save(blob, path)


def test_command_lines_train_features_and_attack(tmp_path, monkeypatch):
    """`train --norm batch -d minimal -a` (one epoch), `evaluate features` and `attack --limit 8` on the run: the stem is the node
    in all three (the attack's image gradient comes through it), every output finite."""
    import csv
    import numpy as np
    from unittest import mock
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import attack as A
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as Tr
    monkeypatch.setattr(nof.ministem.MinimalStem, 'fused_batch', True)
    run, data = str(tmp_path / 'run'), str(tmp_path / 'data.pt')
    _mnist_blob(data)
    fn = nof.ministem._BnMiniStemFn
    with mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        assert Tr.main(['--dataset', 'mnist', '--norm', 'batch', '-d', 'minimal', '-f', '64', '-b', '32', '--data', data, '-a',
                        '--lr', '0.001', '-e', '1', '-t', '1e-2', '--augmentation', 'crop', '--run-dir', run]) == 0
    assert node.call_count >= 2                          # one per batch
    ckpt = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ckpt['params']['norm'] == 'batch' and ckpt['params']['downsample'] == 'minimal'
    assert math.isfinite(ckpt['metrics']['loss'])
    with mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        E.main(['features', run])
    assert node.call_count >= 1
    with np.load(os.path.join(run, 'features.npz')) as f:
        assert np.isfinite(f['features']).all() and f['features'].shape[-1] == 64
    argv = [run, '-t', '1e-2', '-e', '0.5', '-d', 'inf', '-s', '0.1', '--batch-size', '4', '--limit', '8']
    with mock.patch.object(fn, 'apply', wraps=fn.apply) as node:
        path = A.main(['attack'] + argv)
    assert node.call_count >= 2
    with open(path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == list(A.COLUMNS) and len(rows) == 9
    dist = [float(r[list(A.COLUMNS).index('distance')]) for r in rows[1:]]
    assert all(d == d and d >= 0.0 for d in dist), dist            # a distance, or inf where no adversarial was found: never NaN
    assert any(math.isfinite(d) for d in dist), dist

"""GPU: the `norm='batch'` residual stem as one HIP node (stem.py `_BnStemFn`, csrc/bnstem_api.hip: node_bnstem_fwd /
node_bnstem_bwd; reference model.py:167-178, :284-310 with model.py:274), the whole `ResNet(..., norm='batch')` on it and the
command lines that pick it up.

Reference: the same modules as `.double()` on the CPU (tests/bnstem_cases.py), never the node.  Metric: bntrunk_cases.errors --
max-norm error over max|ref| for the output and the image gradient; parameter gradients relative to max(max|ref|, 1e-4 x the
largest gradient) (conv0's bias gradient is zero identically in front of a BatchNorm).  Bound per quantity: max(2e-5, 4 x the same
error of the fp32 modules on the CPU), computed here -- the first term is tests/test_gpu_stem.py's, the second
tests/test_gpu_bnfunc.py's allowance for two correct fp32 summation orders.

Every run asserts `type(out.grad_fn).__name__ == '_BnStemFnBackward'`: without the node the module sequence runs and every test
built on `run_node` fails.

Worst measured error per case on an MI355X (ordinary / kinkfree / split), conv0's bias gradient apart; the quantity is a norm's weight or
bias gradient everywhere but where named; bound 2e-5 where no other is given:
    (1, 28, 64, 2)       9.9e-7 / 3.6e-6 / 4.7e-6        (3, (12, 9), 64, 2)  1.1e-6 / 9.0e-6 / 2.8e-6
    (3, 32, 128, 3)      9.8e-7 / 5.8e-6 / 7.4e-6        (1, (6, 5), 64, 4)   2.7e-6 / 1.4e-5 / 1.8e-5, the last two block 2's conv1 weight
    (3, 32, 256, 2)      1.1e-6 / 1.1e-5 (2.3e-5) / 7.5e-6                        (bounds 1.1e-4 and 2.6e-5 by the second term)
    (3, 32, 192, 2)      1.6e-6 / 4.4e-6 / 4.6e-6        (3, 32, 64, 5)       1.2e-6 / 5.7e-6 / 9.5e-6; the same figures under caps 128 and 1024
    (3, 32, 64, 33)      (no admissible seed) / 1.2e-5 (2.9e-5) / 1.7e-5 (3.6e-5); output 9.0e-7, image gradient 3.4e-7
Output at most 1.6e-6 ((3, 32, 192, 2) kinkfree), image gradient at most 4.3e-6 ((1, (6, 5), 64, 4) kinkfree).
conv0's bias gradient is zero identically in front of a BatchNorm; relative to 1e-4 x the largest gradient it stands at 4.2e-5 .. 2.5e-3
(worst: (3, 32, 64, 5) ordinary), where the fp32 modules on the CPU stand at 5.0e-5 .. 3.4e-3; always inside 4 x the latter.
Whole model (kink-free / split): worst 5.9e-5 / 3.6e-5, conv weight gradients of trunk blocks (the fp32 modules on the CPU: 1.3e-4 / 2.9e-5)."""
import copy
import math
import os

import pytest
import torch

from tests import bnstem_cases as S
from tests import bntrunk_cases as T

pytestmark = pytest.mark.gpu
NODE = '_BnStemFnBackward'


def _id(v):
    if isinstance(v, str):
        return v
    cin, side, f, n = v
    return 'i%d_%s_f%d_n%d' % (cin, '%dx%d' % side if isinstance(side, tuple) else side, f, n)


def run_node(case, mode, stem=None, frozen=False):
    """Forward + backward of the node on the GPU with `input_grad` on: (out, d_x, parameter gradients by name, ())."""
    seed = S.seed_of(case, mode)
    if stem is None:
        stem = S.stem_pair(case, seed, mode)[0]
    stem = stem.cuda()
    stem.input_grad = True
    if frozen:
        for p in stem.parameters():
            p.requires_grad_(False)
    x, cot = S.case_inputs(case, seed)
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == NODE          # the node, not the module sequence
    out.backward(cot.cuda())
    return out.detach(), xg.grad, {k: p.grad for k, p in stem.named_parameters()}, ()


def check_against_fp64(case, mode, got, tag):
    r64, r32 = S.references(case, mode)
    errs, floor = T.errors(got, r64), T.errors(r32, r64)
    assert len(errs) == 2 + 16
    bad = {}
    for k, v in errs.items():
        bnd = S.bound(floor[k])
        print('bnstem %s %s%s: %-32s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (_id(case), mode, tag, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    worst = max(errs, key=errs.get)
    print('bnstem %s %s%s: WORST %s %.2e' % (_id(case), mode, tag, worst, errs[worst]))
    assert not bad, bad


RUNS = [r for case in S.ALL_CASES for r in S.runs(case)]


@pytest.mark.parametrize('case,mode', RUNS, ids=_id)
def test_output_image_gradient_and_every_parameter_gradient_match_fp64(case, mode):
    check_against_fp64(case, mode, run_node(case, mode), '')


def test_frozen_parameters_leave_the_image_gradient_bit_for_bit():
    """grads = NULL: the data-gradient chain alone.  d_x has the bits of the run with parameter gradients; no parameter has a .grad."""
    case, mode = (3, 32, 64, 5), 'ordinary'
    full, frozen = run_node(case, mode), run_node(case, mode, frozen=True)
    assert torch.equal(full[0], frozen[0])
    assert torch.equal(full[1], frozen[1])
    assert all(g is None for g in frozen[2].values()) and all(g is not None for g in full[2].values())


@pytest.mark.parametrize('cap', [128, 1024])
def test_forced_chunk_cap_stays_within_the_bounds(cap, monkeypatch):
    from neural_ode_features_amd import _lib
    case, mode = (3, 32, 64, 5), 'ordinary'
    monkeypatch.setenv('NODE_TUNE_BNSTEM_MAXCHUNK', str(cap))
    n, cin, h, w = S.shape_of(case)
    plan = _lib.bnstem_plan(n, cin, h, w, case[2])
    assert plan[0]['nchunk'] == (71 if cap == 128 else 141) and plan[0]['chunk_rows'] == (64 if cap == 128 else 32)
    check_against_fp64(case, mode, run_node(case, mode), ' cap %d' % cap)


def test_two_runs_return_the_same_bits():
    case, mode = (3, 32, 64, 33), 'kinkfree'
    a, b = run_node(case, mode), run_node(case, mode)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_forwards_in_flight_keep_their_own_workspaces():
    case = (1, 28, 64, 2)
    stem = S.stem_pair(case, 5)[0].cuda()
    stem.input_grad = True
    xs = [S.case_inputs(case, s)[0].cuda() for s in (1, 2, 3)]
    cots = [S.case_inputs(case, s)[1].cuda() for s in (1, 2)]

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
    # the no-grad forward (shared storage, the stream's scratch) returns the bits of the forward that keeps everything
    with torch.no_grad():
        assert torch.equal(stem(xs[2]), stem(xs[2].clone().requires_grad_(True)).detach())


def _modules_match_fp64(stem, ref, x, requires_grad=False):
    """a refused stem ran the module sequence and still matches fp64 (the bounds of test_gpu_stem.py's refusal test)"""
    xg = x.cuda().requires_grad_(requires_grad)
    out = stem(xg)
    assert type(out.grad_fn).__name__ not in (NODE, '_StemFnBackward')
    out_ref = ref(x.double())
    cot = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(9))
    for p in list(stem.parameters()) + list(ref.parameters()):
        p.grad = None
    out.backward(cot.cuda())
    out_ref.backward(cot.double())
    assert float((out.detach().cpu().double() - out_ref.detach()).abs().max() / out_ref.detach().abs().max()) <= 1e-4
    for (name, p), (_, q) in zip(stem.named_parameters(), ref.named_parameters()):
        if name == '0.bias':         # zero identically in front of a BatchNorm: nothing to be relative to
            continue
        assert float((p.grad.cpu().double() - q.grad).norm() / q.grad.norm()) <= 1e-3, name


def test_what_the_node_refuses_runs_the_module_sequence():
    import neural_ode_features_amd as nof
    case = (3, 32, 64, 2)
    stem, ref = S.stem_pair(case, 1)
    stem = stem.cuda()
    x = S.case_inputs(case, 1)[0]
    assert type(stem(x.cuda()).grad_fn).__name__ == NODE
    stem.fused_batch = False
    _modules_match_fp64(stem, ref, x)
    del stem.fused_batch
    try:
        nof.stem.ResidualStem.fused_batch = False
        _modules_match_fp64(stem, ref, x)
    finally:
        nof.stem.ResidualStem.fused_batch = True
    assert type(stem(x.cuda()).grad_fn).__name__ == NODE
    # an input that requires a gradient, input_grad off
    assert stem.input_grad is False
    _modules_match_fp64(stem, ref, x, requires_grad=True)
    # a tracked BatchNorm2d in one slot (training mode: it normalises with the batch's statistics, as the fp64 copy does)
    tracked, tracked_ref = S.stem_pair(case, 1)
    tracked[2].norm1 = torch.nn.BatchNorm2d(64)
    tracked_ref[2].norm1 = torch.nn.BatchNorm2d(64).double()
    _modules_match_fp64(tracked.cuda(), tracked_ref, x)
    # filters = 96
    s96, r96 = S.stem_pair((3, 32, 96, 2), 1)
    _modules_match_fp64(s96.cuda(), r96, x)
    # a 64 x 64 image: 3844 pixels behind the first layer
    x64 = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    _modules_match_fp64(stem, ref, x64)
    # N H2 W2 = 1: what nn.BatchNorm2d raises
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        stem(torch.randn(1, 3, 5, 5, device='cuda'))
    # the GroupNorm stem at the same shape takes the path it took
    gn = nof.ODENet(3, out=10, n_filters=64, downsample='residual', adjoint=True).downsample.module.cuda()
    assert type(gn(x.cuda()).grad_fn).__name__ == '_StemFnBackward'


def test_no_miopen_or_aten_norm_kernel_in_a_fused_step():
    from torch.profiler import ProfilerActivity, profile
    case = (3, 32, 64, 2)
    stem = S.stem_pair(case, 1)[0].cuda()
    stem.input_grad = True
    x = S.case_inputs(case, 1)[0].cuda().requires_grad_(True)
    stem(x).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = stem(x)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('miopen', 'batch_norm', 'igemm', 'batched_transpose'))]
    assert not bad, bad
    assert any('_BnStemFn' in k for k in names), names


# ---------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', S.MODEL_MODES)
def test_whole_model_logits_and_every_gradient_match_fp64(mode):
    """ResNet(3, 64 filters, residual stem, norm='batch') at [4, 3, 32, 32]: stem node, trunk node, BatchNorm head node, Linear."""
    net = S.model_pair(S.KINK_FREE_SEED, mode)[0].cuda()
    for m in net.modules():
        if hasattr(m, 'input_grad'):
            m.input_grad = True            # (run_model asks for the image's gradient)
    x, cot = S.model_inputs(S.KINK_FREE_SEED)
    seen = []
    hooks = [net.downsample.module.register_forward_hook(lambda m, i, o: seen.append(type(o.grad_fn).__name__)),
             net.features.register_forward_hook(lambda m, i, o: seen.append(type(o.grad_fn).__name__))]
    got = T.run_model(net, x.cuda(), cot.cuda())
    for h in hooks:
        h.remove()
    assert seen == [NODE, '_BnTrunkFnBackward']
    r64, r32 = S.model_references(mode)
    errs, floor = T.model_errors(got, r64), T.model_errors(r32, r64)
    bad = {}
    for k, v in errs.items():
        bnd = T.bound(S.MODEL_BLOCKS, floor[k])
        print('bn resnet (residual stem) %s: %-40s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (mode, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    assert not bad, bad


def test_command_lines_train_and_features(tmp_path):
    """`train --model resnet --norm batch` with the default `-d residual` (one epoch, synthetic data), then `evaluate features`."""
    import numpy as np
    from unittest import mock
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as Tr
    run = str(tmp_path / 'run')
    with mock.patch.object(nof.stem._BnStemFn, 'apply', wraps=nof.stem._BnStemFn.apply) as node:
        assert Tr.main(['--model', 'resnet', '--norm', 'batch', '-f', '64', '--synthetic-size', '64', '-b', '32', '-e', '1',
                        '--run-dir', run]) == 0
    assert node.call_count >= 2
    ckpt = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ckpt['params']['norm'] == 'batch' and ckpt['params']['model'] == 'resnet' and ckpt['params']['downsample'] == 'residual'
    assert math.isfinite(ckpt['metrics']['loss'])
    E.main(['features', run])
    with np.load(os.path.join(run, 'features.npz')) as f:
        assert f['features'].shape[1] == 7 and f['features'].shape[-1] == 64
        assert np.isfinite(f['features']).all()


def test_command_line_attack_goes_through_the_node(tmp_path):
    """`attack` on a `train --norm batch -f 64 -a` run of one epoch (the arguments of tests/test_gpu_attack.py's command-line test at
    --limit 8): finite perturbations, and the gradient of the image comes through the node."""
    import csv
    from unittest import mock
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import attack as A
    from neural_ode_features_amd import train as Tr
    run, data = str(tmp_path / 'run'), str(tmp_path / 'data.pt')
    gen = torch.Generator().manual_seed(5)
    blob = dict(x_train=torch.randint(0, 256, (64, 1, 28, 28), generator=gen).to(torch.uint8), y_train=torch.arange(64) % 10,
                x_test=torch.randint(0, 256, (32, 1, 28, 28), generator=gen).to(torch.uint8), y_test=torch.zeros(32, dtype=torch.int64))
    torch.save(blob, data)
    assert Tr.main(['--dataset', 'mnist', '--norm', 'batch', '-f', '64', '-b', '32', '--data', data, '-a', '--lr', '0.001', '-e', '1',
                    '-t', '1e-2', '--augmentation', 'crop', '--run-dir', run]) == 0
    argv = [run, '-t', '1e-2', '-e', '0.5', '-d', 'inf', '-s', '0.1', '--batch-size', '4', '--limit', '8']
    with mock.patch.object(nof.stem._BnStemFn, 'apply', wraps=nof.stem._BnStemFn.apply) as node:
        path = A.main(['attack'] + argv)
    assert node.call_count >= 2
    with open(path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == list(A.COLUMNS) and len(rows) == 9
    dist = [float(r[list(A.COLUMNS).index('distance')]) for r in rows[1:]]
    assert all(d == d and d >= 0.0 for d in dist), dist            # a distance, or inf where no adversarial was found: never NaN
    assert any(math.isfinite(d) for d in dist), dist

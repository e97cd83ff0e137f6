"""GPU: the ResNet baseline's residual trunk as one HIP node (resnet.py, csrc/trunk_api.hip; reference model.py:65-111,
284-310): output, input gradient and every parameter gradient against the same modules run in fp64 on the CPU and
against a fixture the reference wrote; the tapped block outputs; the workspace discipline of forwards in flight; what
PyTorch dispatches; the fallbacks; the whole model; the command lines.

Bounds.  `test_whole_stem_forward_and_every_gradient_match_fp64` holds 2e-5 of max|ref| in max norm for the output and the
gradients through two residual blocks on these very kernels; here the bound is 2e-5 x max(1, blocks / 2): 2e-5 up to two
blocks, 6e-5 at six (rounding errors of successive blocks add).

Seeds of the ordinary-parameter cases (`SEEDS`) were chosen on the CPU: the module sequence runs in fp32 and in fp64, and a
seed is eligible only if EVERY ReLU mask (the sign of every GroupNorm output) agrees between the two; among the eligible
seeds 0..19 of a case the one whose smallest |pre-activation| is largest was kept (`python tests/test_gpu_resnet.py`
prints the table).  A mask that differs on the GPU is then the kernel's doing, not the lottery of a pre-activation within
fp32 rounding of zero.  tests/test_resnet_host.py re-checks the agreement of the seeds kept here without a GPU."""
import copy
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

# (C, side, N, blocks)
CASES = [(64, 8, 2, 1),      # one block, one column tile
         (64, 7, 3, 2),      # MNIST geometry: 147 rows is not a multiple of the 128-row tile, odd batch
         (128, 8, 2, 6),     # full depth, two column tiles, 4 channels per group
         (256, 8, 2, 6),     # the CIFAR width
         (64, 16, 1, 2),     # one-shot-stem states
         (64, 14, 1, 1)]
SEEDS = {(64, 8, 2, 1): 12, (64, 7, 3, 2): 8, (128, 8, 2, 6): 19, (256, 8, 2, 6): 14, (64, 16, 1, 2): 16, (64, 14, 1, 1): 10}
KINK_FREE_SEED = 5


def bound(blocks):
    return 2e-5 * max(1.0, blocks / 2)


def trunk_pair(C, blocks, seed, kink_free=False):
    """(fp32 ResidualTrunk, its fp64 copy): GroupNorm weights and biases perturbed by 0.2 randn; kink-free: the biases in
    front of the ReLUs at +8, so that every pre-activation is positive and no mask can differ."""
    import neural_ode_features_amd as nof
    torch.manual_seed(seed)
    trunk = nof.ResidualTrunk(C, blocks)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in trunk.named_parameters():
            if 'norm' in name:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if kink_free and name.endswith('bias'):
                    p.add_(8.0)
    return trunk, copy.deepcopy(trunk).double()


def case_inputs(case, seed):
    C, side, N, _ = case
    gen = torch.Generator().manual_seed(seed + 2)
    return torch.randn(N, C, side, side, generator=gen), torch.randn(N, C, side, side, generator=gen)


def relu_masks(trunk, x):
    """(the sign of every GroupNorm output of a CPU run, the smallest |pre-activation|)"""
    masks, margin, hooks = [], [float('inf')], []

    def hook(m, i, o):
        masks.append(o > 0)
        margin[0] = min(margin[0], float(o.abs().min()))
    for blk in trunk:
        hooks += [blk.norm1.register_forward_hook(hook), blk.norm2.register_forward_hook(hook)]
    with torch.no_grad():
        torch.nn.Sequential.forward(trunk, x)
    for h in hooks:
        h.remove()
    return masks, margin[0]


def masks_agree(case, seed):
    """(every ReLU mask of the fp32 and the fp64 CPU run agrees, smallest |pre-activation| of the fp64 run)"""
    trunk, ref = trunk_pair(case[0], case[3], seed)
    x, _ = case_inputs(case, seed)
    m32, _ = relu_masks(trunk, x)
    m64, margin = relu_masks(ref, x.double())
    return all(torch.equal(a, b) for a, b in zip(m32, m64)), margin


@functools.lru_cache(maxsize=None)
def fp64_reference(case, seed, kink_free):
    """The fp64 CPU run of a case, computed once and shared: (output, input gradient, parameter gradients by name, block outputs)."""
    _, ref = trunk_pair(case[0], case[3], seed, kink_free)
    x, cot = case_inputs(case, seed)
    xd = x.double().requires_grad_(True)
    taps, h = [], xd
    for blk in ref:
        h = blk(h)
        taps.append(h.detach())
    h.backward(cot.double())
    return h.detach(), xd.grad, {k: p.grad for k, p in ref.named_parameters()}, taps


def rel(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def run_fused(case, seed, kink_free):
    trunk, _ = trunk_pair(case[0], case[3], seed, kink_free)
    trunk = trunk.cuda()
    x, cot = case_inputs(case, seed)
    xg = x.cuda().requires_grad_(True)
    out = trunk(xg)
    assert type(out.grad_fn).__name__ == '_TrunkFnBackward'          # the fused node, not the module sequence
    out.backward(cot.cuda())
    return trunk, xg, out


@pytest.mark.parametrize('kink_free', [False, True], ids=['ordinary', 'kinkfree'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'c%d_%dpx_n%d_b%d' % c)
def test_trunk_output_and_every_gradient_match_fp64(case, kink_free):
    seed = KINK_FREE_SEED if kink_free else SEEDS[case]
    out_ref, dx_ref, grads_ref, _ = fp64_reference(case, seed, kink_free)
    trunk, xg, out = run_fused(case, seed, kink_free)
    errs = {'output': rel(out, out_ref), 'input gradient': rel(xg.grad, dx_ref)}
    for name, p in trunk.named_parameters():
        errs['grad ' + name] = rel(p.grad, grads_ref[name])
    tag = 'trunk (C %d, %dx%d, N %d, %d blocks) %s' % (case[0], case[1], case[1], case[2], case[3], 'kink-free' if kink_free else 'ordinary')
    for k, v in errs.items():
        print('%s: %-26s max error / max|ref| = %.2e' % (tag, k, v))
    worst = max(errs, key=errs.get)
    print('%s: WORST %s %.2e (bound %.1e)' % (tag, worst, errs[worst], bound(case[3])))
    assert errs[worst] <= bound(case[3]), errs


def test_trunk_at_a_batch_that_splits_the_weight_gradient():
    """The cases above have at most 256 pixel rows: ONE split-K share per weight gradient, one or two row tiles per
    convolution.  (64, 8, 64, 2) has 4096 rows -- 64 shares of 64 rows, summed by the reduction launch, and 32 row tiles --
    on kink-free parameters (at this many pre-activations ordinary ones flip masks between any two correct implementations)."""
    case, seed = (64, 8, 64, 2), KINK_FREE_SEED
    out_ref, dx_ref, grads_ref, _ = fp64_reference(case, seed, True)
    trunk, xg, out = run_fused(case, seed, True)
    errs = {'output': rel(out, out_ref), 'input gradient': rel(xg.grad, dx_ref)}
    for name, p in trunk.named_parameters():
        errs['grad ' + name] = rel(p.grad, grads_ref[name])
    worst = max(errs, key=errs.get)
    print('trunk (C 64, 8x8, N 64, 2 blocks) kink-free: WORST %s %.2e (bound %.1e)' % (worst, errs[worst], bound(2)))
    assert errs[worst] <= bound(2), errs


def test_trunk_matches_the_reference_fixture(golden_dir):
    """tests/golden/resnet_trunk2_c64.pt: the reference's own `nn.Sequential(ResBlock(64, 64), ResBlock(64, 64))` on a
    [2, 64, 7, 7] input.  The reference's state_dict loads unchanged; output within 2e-5, gradients within 1e-4 (the
    fixture itself is fp32: PyTorch-CPU's own rounding sits at ~1e-6)."""
    import neural_ode_features_amd as nof
    g = torch.load(os.path.join(golden_dir, 'resnet_trunk2_c64.pt'), map_location='cpu', weights_only=False)
    trunk = nof.ResidualTrunk(64, 2)
    trunk.load_state_dict(g['state_dict'], strict=True)
    assert all(p.dtype == torch.float32 for p in trunk.parameters())
    trunk = trunk.cuda()
    xg = g['x'].cuda().requires_grad_(True)
    out = trunk(xg)
    assert type(out.grad_fn).__name__ == '_TrunkFnBackward'
    out.backward(g['cot'].cuda())
    e = rel(out, g['out'].double())
    print('reference trunk fixture: output %.2e' % e)
    assert e <= 2e-5
    e = rel(xg.grad, g['dx'].double())
    print('reference trunk fixture: input gradient %.2e' % e)
    assert e <= 1e-4
    for name, p in trunk.named_parameters():
        e = rel(p.grad, g['grads'][name].double())
        print('reference trunk fixture: grad %-16s %.2e' % (name, e))
        assert e <= 1e-4, (name, e)


def test_taps_are_the_block_outputs():
    case, seed = (64, 7, 3, 6), KINK_FREE_SEED
    _, _, _, taps_ref = fp64_reference(case, seed, True)
    trunk, _ = trunk_pair(case[0], case[3], seed, True)
    trunk = trunk.cuda()
    x, _ = case_inputs(case, seed)
    with torch.no_grad():
        out, taps = trunk.forward_taps(x.cuda())
        plain = trunk(x.cuda())
    assert len(taps) == 6
    for i, (t, r) in enumerate(zip(taps, taps_ref)):
        e = rel(t, r)
        print('tap %d: max error / max|ref| = %.2e' % (i, e))
        assert e <= bound(6), (i, e)
    assert torch.equal(out, taps[-1]) and torch.equal(out, plain)


def _grads(trunk, xg):
    return [xg.grad.clone()] + [p.grad.clone() for p in trunk.parameters()]


def test_workspace_discipline_of_forwards_in_flight():
    case, seed = (64, 8, 2, 2), 3
    trunk, _ = trunk_pair(case[0], case[3], seed)
    trunk = trunk.cuda()
    xa, ca = (t.cuda() for t in case_inputs(case, seed))
    xb, cb = (t.cuda() for t in case_inputs(case, seed + 10))

    def one(x, cot, between=None):
        trunk.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        out = trunk(xg)
        if between is not None:
            between()
        out.backward(cot)
        return [out.detach().clone()] + _grads(trunk, xg)

    ref_a, ref_b = one(xa, ca), one(xb, cb)
    # the same call twice: identical bits for the output and every gradient
    for u, v in zip(ref_a, one(xa, ca)):
        assert torch.equal(u, v)
    # a no-grad forward (of other data) between a forward and its backward
    def nograd():
        with torch.no_grad():
            trunk(xb)
    for u, v in zip(ref_a, one(xa, ca, nograd)):
        assert torch.equal(u, v)
    # forward A, forward B, backward B, backward A  (gradient accumulation keeps two forwards in flight)
    trunk.zero_grad(set_to_none=True)
    ga, gb = xa.clone().requires_grad_(True), xb.clone().requires_grad_(True)
    oa = trunk(ga)
    ob = trunk(gb)
    ob.backward(cb)
    got_b = [ob.detach().clone()] + _grads(trunk, gb)
    trunk.zero_grad(set_to_none=True)
    oa.backward(ca)
    got_a = [oa.detach().clone()] + _grads(trunk, ga)
    for u, v in zip(ref_a + ref_b, got_a + got_b):
        assert torch.equal(u, v)
    # a second backward through one forward raises instead of reading a workspace that was handed on
    out = trunk(xa.clone().requires_grad_(True))
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        out.sum().backward()


def test_trunk_runs_no_library_convolution():
    """As test_stem_runs_no_library_convolution: PyTorch dispatches no convolution, no GroupNorm, no ReLU and no layout
    transpose for a forward + backward of the fused trunk."""
    from torch.profiler import ProfilerActivity, profile
    trunk, _ = trunk_pair(64, 2, seed=7)
    trunk = trunk.cuda()
    x = torch.randn(2, 64, 8, 8).cuda().requires_grad_(True)
    trunk(x).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        out = trunk(x)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('conv', 'miopen', 'group_norm', 'native_group_norm', 'transpose', 'relu'))]
    assert not bad, bad
    assert any('_TrunkFn' in k for k in names), names


@pytest.mark.parametrize('where', ['c96', 'c32', 'cpu'])
def test_shapes_the_kernels_refuse_run_the_module_sequence(where):
    C = {'c96': 96, 'c32': 32, 'cpu': 64}[where]
    case = (C, 8, 2, 2)
    trunk, ref = trunk_pair(C, 2, seed=11, kink_free=True)
    x, cot = case_inputs(case, 11)
    if where != 'cpu':
        trunk, x, cot = trunk.cuda(), x.cuda(), cot.cuda()
    xg = x.requires_grad_(True)
    out = trunk(xg)
    assert type(out.grad_fn).__name__ != '_TrunkFnBackward'
    out.backward(cot)
    xd = x.detach().cpu().double().requires_grad_(True)
    out_ref = ref(xd)
    out_ref.backward(cot.cpu().double())
    assert rel(out, out_ref.detach()) <= 1e-4
    assert rel(xg.grad, xd.grad) <= 1e-4
    for (name, p), (_, q) in zip(trunk.named_parameters(), ref.named_parameters()):
        assert rel(p.grad, q.grad) <= 1e-4, name


def test_whole_model_matches_fp64():
    """`ResNet(3, n_filters=64, downsample='residual')` at N = 4, 32x32, kink-free parameters: logits and every parameter
    gradient of a cross-entropy backward.  Eight residual blocks lie between image and logits: 2e-5 x 8 / 2 = 8e-5."""
    import torch.nn.functional as F
    import neural_ode_features_amd as nof
    torch.manual_seed(21)
    net = nof.ResNet(3, n_filters=64, downsample='residual')
    gen = torch.Generator().manual_seed(22)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if 'norm' in name or name.startswith('classifier.module.0'):
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if name.endswith('bias'):
                    p.add_(8.0)
    ref = copy.deepcopy(net).double()
    net = net.cuda()
    x = torch.randn(4, 3, 32, 32, generator=gen)
    y = torch.tensor([1, 9, 0, 4])
    logits = net(x.cuda())
    F.cross_entropy(logits, y.cuda()).backward()
    logits_ref = ref(x.double())
    F.cross_entropy(logits_ref, y).backward()
    errs = {'logits': rel(logits, logits_ref.detach())}
    for (name, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        errs['grad ' + name] = rel(p.grad, q.grad)
    for k, v in errs.items():
        print('whole ResNet (3 -> 64 filters, residual stem, N 4): %-44s max error / max|ref| = %.2e' % (k, v))
    worst = max(errs, key=errs.get)
    print('whole ResNet: WORST %s %.2e (bound 8.0e-05)' % (worst, errs[worst]))
    assert errs[worst] <= 8e-5, errs
    # feature extraction: the fused forward's taps against the module sequence (block by block, fp64)
    net.eval().to_features_extractor()
    ref.eval().to_features_extractor()
    with torch.no_grad():
        feats, feats_ref = net(x.cuda()), ref(x.double())
    assert tuple(feats.shape) == (7, 4, 64)
    e = rel(feats, feats_ref)
    print('whole ResNet: [7, 4, 64] features max error / max|ref| = %.2e' % e)
    assert e <= 8e-5


def test_command_lines_train_features_retrieval(tmp_path):
    """One epoch of `train --model resnet` on a synthetic --data file, then `evaluate features` / `retrieval` on the run;
    `evaluate nfe` refuses a ResNet run."""
    import numpy as np
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    gen = torch.Generator().manual_seed(31)
    data = tmp_path / 'data.pt'
    torch.save({'x_train': torch.randn(64, 1, 28, 28, generator=gen), 'y_train': torch.arange(64) % 10,
                'x_test': torch.randn(32, 1, 28, 28, generator=gen), 'y_test': torch.arange(32) % 10}, data)
    run = str(tmp_path / 'run')
    assert T.main(['--model', 'resnet', '--dataset', 'mnist', '-d', 'residual', '-f', '64', '-e', '1', '-b', '32', '--lr', '0.01',
                   '--data', str(data), '--run-dir', run]) == 0
    ckpt = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ckpt['params']['model'] == 'resnet'
    assert ckpt['metrics']['nfe-f'] == 0 and ckpt['metrics']['nfe-b'] == 0 and ckpt['metrics']['test_nfe'] == 0
    assert any(k.startswith('features.5.conv2') for k in ckpt['model'])
    E.main(['features', run])
    with np.load(os.path.join(run, 'features.npz')) as f:
        assert f['features'].shape == (1, 7, 32, 64)
        assert np.allclose(f['t1s'], np.linspace(0, 1, 7)) and list(f['tols']) == [0]
        assert np.isfinite(f['features']).all()
    E.main(['retrieval', run])
    assert os.path.exists(os.path.join(run, 'retrieval.csv'))
    with pytest.raises(SystemExit, match='ResNet'):
        E.main(['nfe', run])


if __name__ == '__main__':      # the seed table of the docstring (CPU only)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for case in CASES:
        rows = [(s,) + masks_agree(case, s) for s in range(20)]
        ok = [(m, s) for s, agree, m in rows if agree]
        print(case, 'eligible seeds:', [s for _, s in ok], '-> kept', max(ok)[1], 'smallest |pre-activation| %.2e' % max(ok)[0])

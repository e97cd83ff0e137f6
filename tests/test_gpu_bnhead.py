"""GPU: the `norm='batch'` classifier head as two HIP launches each way (head.py `bn_head_pool`, csrc/kernels_bnhead.hip,
csrc/bnhead_api.hip: node_bnhead_fwd / node_bnhead_bwd; reference model.py:231-250 with model.py:274).

Reference: BatchNorm2d(track_running_stats=False) -> ReLU -> AdaptiveAvgPool2d -> scale as `.double()` modules on the CPU
(tests/bnhead_cases.py).  Metric: max-norm error over max|ref|.  Bounds: pooled 1e-5, dz / dgamma / dbeta 2e-5 (those
tests/test_gpu_head.py holds the GroupNorm head to), each widened to 4 x the fp32 CPU modules' own error where that is larger,
computed here.  Every case runs with and without a dropout scale; the x = 50 + randn case is there for E[x^2] - E[x]^2.

Worst measured error per shape on an MI355X over the three parameter sets, with and without dropout (pooled / dz / dgamma / dbeta):
    (2, 64, 8, 8)    9.8e-8 / 2.0e-7 / 2.1e-7 / 3.6e-8        (2, 256, 8, 8)   < 1e-7 / 2.3e-7 / 1.4e-7 / 5.5e-8
    (3, 64, 7, 7)    < 1e-7 / 2.3e-7 / 1.8e-7 / 6.3e-8        (84, 64, 7, 7)   < 1e-7 / 2.2e-7 / 1.1e-7 / 5.6e-8
    (2, 192, 8, 8)   < 1e-7 / 2.2e-7 / 2.1e-7 / 4.0e-8        (1, 64, 6, 5)    ordinary: < 1e-7 / 3.0e-7 / 1.3e-7 / 6.1e-8
    (4, 64, 8, 8) at x = 50 + randn: 3.2e-6 / 4.7e-6 / 2.9e-5 / 4.4e-8 -- dgamma kink-free without dropout, where the fp32 modules on the CPU
    stand at 1.1e-5 (bound 4.5e-5 by the second term): an fp32 input of size 50 carries 3e-6 of the spread in its own rounding.
    (1, 64, 6, 5) kink-free and split: dz and dgamma vanish identically (bnhead_cases.errors says how they are scaled).
Every run prints its errors (`-s`)."""
import pytest
import torch
from torch import nn

from tests import bnhead_cases as H

pytestmark = pytest.mark.gpu
NODE = '_BnHeadPoolBackward'


def run_node(case, mode, dropout):
    from neural_ode_features_amd import head
    seed = H.seed_of(case, mode)
    bn = H.norm_pair(case, seed, mode)[0].cuda()
    z, cot, scale = H.case_inputs(case, seed)
    zg = z.cuda().requires_grad_(True)
    assert head.bn_head_fusable(zg, bn)
    pooled = head._BnHeadPool.apply(zg, bn.weight, bn.bias, scale.cuda() if dropout else None, bn.eps)
    assert type(pooled.grad_fn).__name__ == NODE
    pooled.backward(cot.cuda())
    return pooled.detach(), zg.grad, bn.weight.grad, bn.bias.grad


def check(case, mode, dropout):
    r64, r32, S = H.references(case, mode, dropout)
    errs, floor = H.errors(run_node(case, mode, dropout), r64, S), H.errors(r32, r64, S)
    bad = {}
    for k, v in errs.items():
        bnd = max(H.FLOORS[k], 4 * floor[k])
        print('bnhead %s %s %s: %-7s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)'
              % (case, mode, 'dropout' if dropout else 'no dropout', k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    assert not bad, bad


@pytest.mark.parametrize('dropout', [False, True], ids=['plain', 'dropout'])
@pytest.mark.parametrize('mode', H.MODES)
@pytest.mark.parametrize('case', H.CASES + [H.OFFSET_CASE], ids=lambda c: 'n%d_c%d_%dx%d' % c)
def test_pooled_and_every_gradient_match_fp64(case, mode, dropout):
    check(case, mode, dropout)


def test_two_runs_return_the_same_bits():
    a, b = run_node((84, 64, 7, 7), 'ordinary', True), run_node((84, 64, 7, 7), 'ordinary', True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_classifier_takes_the_node_and_its_switch_and_refusals_the_modules():
    import neural_ode_features_amd as nof
    torch.manual_seed(0)
    clf = nof.FCClassifier(64, norm='batch').cuda()
    x = torch.randn(3, 64, 7, 7, device='cuda', requires_grad=True)
    pooled = clf.pooled(x)
    assert type(pooled.grad_fn).__name__ == NODE
    out = clf(x)
    want = clf.module(x)
    assert float((out - want).detach().abs().max()) <= 1e-5 * float(want.detach().abs().max())
    seen = []
    handle = clf.module[0].register_forward_hook(lambda m, i, o: seen.append(1))      # a hook on the norm: the module runs, and is seen
    clf(x)
    handle.remove()
    assert seen == [1]
    clf.fused_batch = False
    assert torch.equal(clf(x), want)
    del clf.fused_batch
    # C = 96, running statistics: the module sequence
    for other, c in ((nof.FCClassifier(96, norm='batch').cuda(), 96), (nof.FCClassifier(64, norm='batch').cuda(), 64)):
        if c == 64:
            other.module[0] = nn.BatchNorm2d(64).cuda()
        xi = torch.randn(2, c, 8, 8, device='cuda')
        from unittest import mock
        from neural_ode_features_amd import head
        with mock.patch.object(head._BnHeadPool, 'apply', side_effect=AssertionError('the node was called')):
            assert other(xi).shape == (2, 10)
    # N H W = 1: what nn.BatchNorm2d raises
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        clf.train()(torch.randn(1, 64, 1, 1, device='cuda'))


def test_dropout_draws_what_the_module_sequence_draws():
    import neural_ode_features_amd as nof
    torch.manual_seed(0)
    clf = nof.FCClassifier(64, dropout=0.5, norm='batch').cuda().train()
    x = torch.randn(4, 64, 8, 8, device='cuda')
    torch.manual_seed(11)
    fused = clf.pooled(x)
    assert type(fused.grad_fn).__name__ == NODE
    torch.manual_seed(11)
    mods = clf.module[:5](x)
    assert torch.equal(fused == 0, mods == 0) and 0.3 < float((fused == 0).float().mean()) < 0.7
    assert float((fused - mods).detach().abs().max()) <= 1e-5 * float(mods.detach().abs().max())
    clf.eval()
    assert not (clf.pooled(x) == 0).any()

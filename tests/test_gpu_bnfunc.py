"""GPU: `ODEfunc(C, norm='batch')` as one HIP node (bnfunc.py, csrc/bnfunc_api.hip, csrc/kernels_batchnorm.hip; reference
model.py:326-348 with model.py:274 and model.py:313-323): output, d_x, d_t and every parameter gradient against the same modules
run in fp64 on the CPU with an fp64 `t` (never against the node itself); statistics of an input with a large mean; the time
argument; bit-reproducibility; the workspace discipline of forwards in flight; what PyTorch dispatches; the generic solver on
top of the node against the oracle; the fallbacks; the command lines.

Metric and bounds (tests/bnfunc_cases.py: `errors`, `bias_ratio`).  Max-norm error over max|ref| for the output, d_x and d_t;
parameter gradients relative to max(max|ref|, 1e-4 x the largest gradient).  Bound per quantity: max(2e-5, 4 x the same error
of the fp32 module operations on the CPU), computed in the test: 2e-5 is this project's bound for two convolutions plus norms on
these kernels (tests/test_gpu_resnet.py::bound), the factor 4 allows for two correct fp32 summation orders differing (it matters for
d_t at 4096 rows, where the CPU fp32 run itself is 1.6e-5 off).  The two convolution biases stand in front of a BatchNorm: their
gradient is zero identically, the node returns the computed sum (rounding noise, not a literal zero), and the test holds
|got[c]| <= 1e-5 x S[c] with S[c] = sum |dL/d(conv output)| of the fp64 run (the fp32 modules sit at <= 1.6e-7 x S).

Ordinary-parameter runs use seeds chosen on the CPU so that no ReLU mask can differ for a reason other than the kernels
(tests/bnfunc_cases.py; tests/test_bnfunc_host.py re-checks them without a GPU).

Measured on an MI355X, worst quantity of each case (ordinary / kink-free); conv biases <= 2.4e-7 x S everywhere:
    (2, 64, 8, 8)    grad norm2.weight 9.1e-7 / grad norm1.bias 3.4e-6      (2, 192, 8, 8)   d_t 1.8e-6 / grad norm1.bias 4.4e-6
    (3, 64, 7, 7)    d_x 7.4e-7 / grad norm1.bias 1.9e-6                    (2, 256, 8, 8)   d_t 3.8e-6 / output 4.4e-6
    (1, 64, 6, 5)    output 7.5e-7 / output 1.7e-6                          (1, 64, 16, 16)  output 1.0e-6 / d_t 2.8e-6
    (2, 128, 8, 8)   grad norm1.bias 1.3e-6 / grad norm1.bias 3.3e-6        (64, 64, 8, 8)   d_t 6.7e-6 / grad norm1.bias 4.0e-6
    x = 50 + randn: output 2.0e-6;  t = 0: grad norm1.bias 2.8e-6;  t = 1: grad norm1.bias 3.1e-6
(d_t of (64, 64, 8, 8) ordinary was 5.6e-5 with fp32 sums behind it: kernels_batchnorm.hip, k_bn_bwd_stats / k_bn_bwd_dx, says what changed.)

Every case above runs chunks of 32 rows: one trip of the passes' row loops.  B.MULTI_CASES are the regimes beyond it (multi-row
chunks, short last chunks, 8 and 16 column tiles, split counts that divide k_bn_reduce's lanes), under three parameter sets; the
'split' set masks every odd channel on every row, so conv1's bias gradient must be an exact zero there (S[c] == 0).  Measured on an
MI355X, worst quantity of each case (ordinary / kink-free / split); conv biases <= 2.7e-7 x S everywhere, exact zeros where S is zero:
    (5, 64, 8, 8)     output 1.0e-6 / output 2.0e-6 / d_t 4.4e-6
    (84, 64, 7, 7)    grad norm2.bias 1.8e-6 / grad norm2.bias 4.5e-6 / grad norm1.bias 5.0e-6
    (33, 256, 8, 8)   grad norm1.bias 3.2e-6 / grad norm2.bias 8.8e-6 / grad norm1.bias 8.9e-6
    (43, 192, 8, 8)   d_t 3.9e-6 / grad norm1.bias 6.5e-6 / grad norm1.bias 7.7e-6
    (2, 512, 4, 4)    grad norm2.weight 3.3e-6 / grad norm2.weight 4.1e-6 / output 4.9e-6
    (17, 512, 8, 8)   grad norm1.bias 4.6e-6 / grad norm1.bias 1.2e-5 / grad norm1.bias 1.1e-5
    (9, 1024, 8, 8)   (no admissible seed) / grad norm1.bias 1.4e-5 / grad norm1.bias 1.4e-5
    (168, 64, 7, 7)   grad norm1.bias 1.7e-6 / grad norm1.bias 5.6e-6 / grad norm1.bias 5.7e-6
(grad norm1.bias grows with the width: 1.4e-5 at C = 1024 against the bound's floor of 2e-5, where the fp32 modules on the CPU stand at
1.4e-6.  C >= 2048 is not tested: the fp64 reference of its two filters and their gradients needs about 1 GB.)
Every subset of wanted gradients returns the bits of the run that wants them all, at (5, 64, 8, 8) and (84, 64, 7, 7).
With the centred pass of k_bn_stats, or the class accumulators of k_bn_bwd_dx<true>, cut to the first trip, every multi-row case here
fails by O(1) (d_x, d_t) while every case of B.CASES passes; with k_bn_reduce's slab loop entered by all four lanes or none, (5, 64, 8, 8)
loses a slab (conv weight gradients off by 0.5 .. 0.9) and every other case passes; with the norm3 stage of node_bnfunc_bwd keeping
its time sums only when parameters are wanted, the subsets without parameters return another problem's d_t (0.54 for 1.60)."""
import copy
import os

import pytest
import torch

from tests import bnfunc_cases as B

pytestmark = pytest.mark.gpu


def run_node(case, seed, kink_free, t=B.T_EVAL, offset=0.0, t_as_float=False, mode=None):
    """Forward + backward of the node on the GPU: (out, d_x, d_t, parameter gradients by name)."""
    func, _ = B.func_pair(case[1], seed, kink_free, mode)
    func = func.cuda()
    x, cot = B.case_inputs(case, seed, offset)
    xg = x.cuda().requires_grad_(True)
    tg = float(t) if t_as_float else torch.tensor(t, dtype=torch.float32, device='cuda').requires_grad_(True)
    out = func(tg, xg)
    assert type(out.grad_fn).__name__ == '_BatchOdeFnBackward'          # the node, not the module operations
    out.backward(cot.cuda())
    return out.detach(), xg.grad, None if t_as_float else tg.grad, {k: p.grad for k, p in func.named_parameters()}


def check_against_fp64(tag, got, refs):
    r64, r32 = refs
    errs = B.errors(got, r64)
    floor = B.errors(r32[:4], r64)
    bad = {}
    for k, v in errs.items():
        bnd = max(2e-5, 4 * floor[k])
        print('%s: %-26s max error / scale = %.2e   (fp32 modules on the CPU %.2e, bound %.1e)' % (tag, k, v, floor[k], bnd))
        if not v <= bnd:
            bad[k] = (v, bnd)
    ratio = B.bias_ratio(got[3], r64)
    print('%s: %-26s max |d bias| / S = %.2e   (fp32 modules on the CPU %.2e, bound 1.0e-05)' % (tag, 'conv biases', ratio, B.bias_ratio(r32[3], r64)))
    worst = max(errs, key=errs.get)
    print('%s: WORST %s %.2e' % (tag, worst, errs[worst]))
    assert not bad, bad
    assert B.bias_within(got[3], r64, 1e-5), ratio      # |got[c]| <= 1e-5 x S[c] channel by channel: an exact zero where S[c] == 0


@pytest.mark.parametrize('kink_free', [False, True], ids=['ordinary', 'kinkfree'])
@pytest.mark.parametrize('case', B.CASES, ids=lambda c: 'n%d_c%d_%dx%d' % c)
def test_node_output_and_every_gradient_match_fp64(case, kink_free):
    seed = B.KINK_FREE_SEED if kink_free else B.SEEDS[case]
    tag = 'bnfunc (N %d, C %d, %dx%d) %s' % (case + ('kink-free' if kink_free else 'ordinary',))
    check_against_fp64(tag, run_node(case, seed, kink_free), B.references(case, seed, kink_free))


MULTI_RUNS = [(case, mode) for case in B.MULTI_CASES for mode in B.MODES if mode != 'ordinary' or case in B.MULTI_SEEDS]


@pytest.mark.parametrize('case,mode', MULTI_RUNS, ids=lambda v: v if isinstance(v, str) else 'n%d_c%d_%dx%d' % v)
def test_multi_row_chunks_wide_channels_and_split_counts_match_fp64(case, mode):
    """The launch regimes of B.MULTI_CASES (tests/test_bnfunc_host.py asserts them through node_bnfunc_describe): second and third
    trips of the passes' row loops, short last chunks, 8 and 16 column tiles, split counts that put k_bn_reduce's lanes on
    different lines.  The check and its bounds are those of the test above, unchanged."""
    seed = B.MULTI_SEEDS[case] if mode == 'ordinary' else B.KINK_FREE_SEED
    tag = 'bnfunc (N %d, C %d, %dx%d) %s' % (case + (mode,))
    check_against_fp64(tag, run_node(case, seed, False, mode=mode), B.references(case, seed, False, mode=mode))


def _run_subset(case, seed, mode, want_t, want_x, want_p):
    func, _ = B.func_pair(case[1], seed, mode=mode)
    func = copy.deepcopy(func).cuda().requires_grad_(want_p)
    x, cot = B.case_inputs(case, seed)
    xg = x.cuda().requires_grad_(want_x)
    tg = torch.tensor(B.T_EVAL, dtype=torch.float32, device='cuda').requires_grad_(want_t)
    out = func(tg, xg)
    assert type(out.grad_fn).__name__ == '_BatchOdeFnBackward'
    out.backward(cot.cuda())
    return out.detach(), xg.grad, tg.grad, {k: p.grad for k, p in func.named_parameters()}


@pytest.mark.parametrize('case,mode', [((5, 64, 8, 8), 'kinkfree'), ((84, 64, 7, 7), 'split')], ids=['n5_kinkfree', 'n84_split'])
def test_every_subset_of_wanted_gradients_returns_the_bits_of_the_full_backward(case, mode):
    """node_bnfunc_bwd branches on what is wanted: k_bn_bwd_dx<false> against <true>, k_bn_reduce without its parameter blocks,
    the skipped norm1 stage.  Both instances of the dx pass round alike and no sum's order depends on the subset, so every
    returned gradient is bit for bit the one of the run that wants everything; an unwanted one is None.
    A workspace is handed from one backward to the next forward of its shape, so a sum that a subset's branch forgot to write
    would be read as the last run left it -- the right bits, if that run had the same data.  Hence the full run of OTHER data in
    front of every subset: what a subset finds in its workspace is another problem's."""
    seed = B.KINK_FREE_SEED
    full = _run_subset(case, seed, mode, True, True, True)
    for bits in range(1, 8):
        want_t, want_x, want_p = bool(bits & 1), bool(bits & 2), bool(bits & 4)
        other = _run_subset(case, seed + 1, mode, True, True, True)
        assert not torch.equal(other[2], full[2])
        out, dx, dt, grads = _run_subset(case, seed, mode, want_t, want_x, want_p)
        tag = 't' * want_t + 'x' * want_x + 'p' * want_p
        assert torch.equal(out, full[0]), tag
        assert (dt is not None) == want_t and (dx is not None) == want_x, tag
        assert all((g is not None) == want_p for g in grads.values()), tag
        if want_t:
            assert torch.equal(dt, full[2]), tag
        if want_x:
            assert torch.equal(dx, full[1]), tag
        if want_p:
            for k in grads:
                assert torch.equal(grads[k], full[3][k]), (tag, k)


def test_statistics_of_an_input_with_a_large_mean():
    """x = 50 + randn: E[x^2] - E[x]^2 in fp32 loses the variance to cancellation (2.7e-4 of max|y| against fp64, an order of magnitude
    over the bound); centred second moments per chunk, combined by Chan's formula, do not."""
    case, seed = B.OFFSET_CASE, B.KINK_FREE_SEED
    check_against_fp64('bnfunc (N 4, C 64, 8x8) kink-free, x = 50 + randn', run_node(case, seed, True, offset=50.0),
                       B.references(case, seed, True, B.T_EVAL, 50.0))


@pytest.mark.parametrize('t', [0.0, 1.0])
def test_time_argument(t):
    case, seed = (2, 64, 8, 8), B.KINK_FREE_SEED
    got = run_node(case, seed, True, t=t)
    check_against_fp64('bnfunc (N 2, C 64, 8x8) kink-free, t = %g' % t, got, B.references(case, seed, True, t))
    # t as a Python float: the same evaluation bit for bit (there is no d_t then)
    out, dx, dt, grads = run_node(case, seed, True, t=t, t_as_float=True)
    assert dt is None
    assert torch.equal(out, got[0]) and torch.equal(dx, got[1])
    for k in grads:
        assert torch.equal(grads[k], got[3][k]), k


def test_results_are_the_same_bits_on_every_run():
    case, seed = (64, 64, 8, 8), B.KINK_FREE_SEED
    first = run_node(case, seed, True)
    for _ in range(2):
        again = run_node(case, seed, True)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])
        for k in first[3]:
            assert torch.equal(first[3][k], again[3][k]), k


def test_non_finite_input_gives_non_finite_output_and_nothing_else():
    """The generic solver also evaluates the function on stage states of steps past the end of the interval, which may be
    non-finite: the node then returns non-finite values (the statistics of a batch hold every sample) and raises nothing."""
    func, _ = B.func_pair(64, 3)
    func = func.cuda()
    x = torch.randn(2, 64, 8, 8, device='cuda')
    x[1, 5, 2, 3] = float('nan')
    xg = x.requires_grad_(True)
    out = func(torch.tensor(0.5, device='cuda'), xg)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert not torch.isfinite(out).any() and not torch.isfinite(xg.grad).any()


def _grads(func, xg, tg):
    return [xg.grad.clone(), tg.grad.clone()] + [p.grad.clone() for p in func.parameters()]


def test_workspace_discipline_of_forwards_in_flight():
    case, seed = (2, 64, 8, 8), 3
    func, _ = B.func_pair(case[1], seed)
    func = func.cuda()
    xa, ca = (v.cuda() for v in B.case_inputs(case, seed))
    xb, cb = (v.cuda() for v in B.case_inputs(case, seed + 10))
    t = torch.tensor(0.37, device='cuda')

    def start(x):
        xg, tg = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
        return xg, tg, func(tg, xg)

    def one(x, cot, between=None):
        func.zero_grad(set_to_none=True)
        xg, tg, out = start(x)
        if between is not None:
            between()
        out.backward(cot)
        return [out.detach().clone()] + _grads(func, xg, tg)

    ref_a, ref_b = one(xa, ca), one(xb, cb)
    # a no-grad forward (of other data) between a forward and its backward: it runs the node and keeps nothing
    def nograd():
        from neural_ode_features_amd import bnfunc
        free = {k: len(v) for k, v in bnfunc._FREE.items()}
        with torch.no_grad():
            out = func(t, xb)
        assert out.grad_fn is None and torch.equal(out, ref_b[0])
        assert {k: len(v) for k, v in bnfunc._FREE.items()} == free
    for u, v in zip(ref_a, one(xa, ca, nograd)):
        assert torch.equal(u, v)
    # forward A, forward B, then the backwards in either order
    for b_first in (True, False):
        func.zero_grad(set_to_none=True)
        ga, ta, oa = start(xa)
        gb, tb, ob = start(xb)
        got = {}
        for which in (('b', 'a') if b_first else ('a', 'b')):
            func.zero_grad(set_to_none=True)
            if which == 'a':
                oa.backward(ca)
                got['a'] = [oa.detach().clone()] + _grads(func, ga, ta)
            else:
                ob.backward(cb)
                got['b'] = [ob.detach().clone()] + _grads(func, gb, tb)
        for u, v in zip(ref_a + ref_b, got['a'] + got['b']):
            assert torch.equal(u, v)
    # a second backward through one forward raises instead of reading a workspace that was handed on
    out = func(t, xa.clone().requires_grad_(True))
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        out.sum().backward()
    # a saliency caller: the input gradient alone
    frozen = copy.deepcopy(func).requires_grad_(False)
    xg = xa.clone().requires_grad_(True)
    frozen(t, xg).backward(ca)
    assert torch.equal(xg.grad, ref_a[1]) and all(p.grad is None for p in frozen.parameters())


def test_node_runs_no_library_operation():
    """As tests/test_gpu_resnet.py::test_trunk_runs_no_library_convolution: PyTorch dispatches no convolution, no batch norm, no
    concatenation, no ReLU and no layout transpose for a forward + backward of the node."""
    from torch.profiler import ProfilerActivity, profile
    func, _ = B.func_pair(64, seed=7)
    func = func.cuda()
    x = torch.randn(2, 64, 8, 8).cuda().requires_grad_(True)
    t = torch.tensor(0.37, device='cuda').requires_grad_(True)
    func(t, x).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        out = func(t, x)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if '_BatchOdeFn' not in k and any(s in k.lower() for s in ('conv', 'miopen', 'batch_norm', 'cat', 'transpose', 'relu'))]
    assert not bad, bad
    assert any('_BatchOdeFn' in k for k in names), names


# ---------------------------------------------------------------------------------------------------------------------
# through the solver (helpers as in tests/test_gpu_generic.py)
# ---------------------------------------------------------------------------------------------------------------------
def _same_nfe(hip, ref, intervals=1):
    """Equal counters -- or one accept / reject decision apart per solve (six evaluations; the backward runs one solve per time
    interval): two fp32 implementations may land on different sides of an error ratio of 1."""
    (hf, hb), (rf, rb) = hip, ref
    df, db = abs(hf - rf), abs((hb - hf) - (rb - rf))
    return df % 6 == 0 and df <= 6 and db % 6 == 0 and db <= 6 * intervals


def _grads_close(hip, ref, bound):
    """Every parameter gradient against the oracle's, each relative to max(its own scale, 1e-4 x the largest gradient of the
    function): a conv bias in front of a normalisation layer has an exactly-zero gradient -- both sides then hold rounding noise only."""
    gmax = max(float(r.abs().max()) for r in ref)
    for g, r in zip(hip, ref):
        g = torch.zeros_like(r) if g is None else g
        scale = max(float(r.abs().max()), 1e-4 * gmax)
        assert float((g - r).abs().max()) / scale < bound, (float((g - r).abs().max()), scale)


def _rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _solve(mod, dev, solve, y, tpts, tol, wgt):
    mod.nfe = 0
    for prm in mod.parameters():
        prm.grad = None
    y0 = y.detach().clone().to(dev).requires_grad_(True)
    out = solve(mod, y0, torch.tensor(tpts).to(dev), rtol=tol, atol=tol, method='dopri5')
    nfe_f = mod.nfe
    (out * wgt.to(dev)).sum().backward()
    return dict(out=out.detach().cpu(), gy=y0.grad.cpu(), gp=[None if p.grad is None else p.grad.cpu() for p in mod.parameters()],
                nfe=(nfe_f, mod.nfe), steps=(getattr(mod, 'last_forward_stats', {}).get('accepted'), getattr(mod, 'last_backward_stats', {}).get('accepted')))


@pytest.mark.parametrize('tpts', [(0.0, 1.0), (0.0, 0.3, 0.55, 1.0)])
def test_generic_solver_on_the_node_against_the_oracle(tpts):
    import neural_ode_features_amd as nof
    from oracle import torchdiffeq_restated as tdq
    tol = 1e-3
    torch.manual_seed(3)
    func = nof.ODEfunc(64, norm='batch')
    y = torch.randn(4, 64, 6, 6, generator=torch.Generator().manual_seed(4))
    wgt = torch.randn((len(tpts),) + tuple(y.shape), generator=torch.Generator().manual_seed(7)) / y[0].numel() ** 0.5
    twin = copy.deepcopy(func).cpu()
    f = func.cuda()
    from unittest import mock
    from neural_ode_features_amd import bnfunc
    with mock.patch.object(bnfunc, 'evaluate', wraps=bnfunc.evaluate) as node:
        hip = _solve(f, 'cuda', nof.odeint_adjoint, y, tpts, tol, wgt)
    calls = node.call_args_list
    assert len(calls) >= hip['nfe'][1] > 0            # every counted evaluation (and the discarded ones past the interval's end) was the node
    ref = _solve(twin, 'cpu', tdq.odeint_adjoint, y, tpts, tol, wgt)
    n = len(tpts) - 1
    assert torch.equal(hip['out'][0], y)
    assert float((hip['out'] - ref['out']).abs().max()) <= 10 * tol
    assert _same_nfe(hip['nfe'], ref['nfe'], n), (hip['nfe'], ref['nfe'])
    assert _rel_err(hip['gy'], ref['gy']) < 2e-2
    _grads_close(hip['gp'], ref['gp'], 2e-2)
    # the same solve on the module operations
    try:
        nof.ODEfunc.fused_batch = False
        mods = _solve(f, 'cuda', nof.odeint_adjoint, y, tpts, tol, wgt)
    finally:
        nof.ODEfunc.fused_batch = True
    print('tpts %s: NFE node %s modules %s oracle %s; accepted steps node %s modules %s' % (tpts, hip['nfe'], mods['nfe'], ref['nfe'], hip['steps'], mods['steps']))
    assert _same_nfe(hip['nfe'], mods['nfe'], n), (hip['nfe'], mods['nfe'])
    assert abs(hip['steps'][0] - mods['steps'][0]) <= 1 and abs(hip['steps'][1] - mods['steps'][1]) <= n, (hip['steps'], mods['steps'])
    assert float((hip['out'] - mods['out']).abs().max()) <= 10 * tol


@pytest.mark.parametrize('C', [16, 96])
def test_shapes_the_kernels_refuse_run_the_module_operations(C):
    case, seed = (2, C, 8, 8), 11
    func, _ = B.func_pair(C, seed, True)
    func = func.cuda()
    x, cot = B.case_inputs(case, seed)
    xg = x.cuda().requires_grad_(True)
    tg = torch.tensor(B.T_EVAL, device='cuda').requires_grad_(True)
    out = func(tg, xg)
    assert type(out.grad_fn).__name__ != '_BatchOdeFnBackward'
    out.backward(cot.cuda())
    r64, _ = B.references(case, seed, True)
    errs = B.errors((out.detach(), xg.grad, tg.grad, {k: p.grad for k, p in func.named_parameters()}), r64)
    assert max(errs.values()) <= 1e-4, errs


def test_command_lines_train_and_features(tmp_path):
    """`train --norm batch` (one epoch, synthetic data), then `evaluate features` on the run."""
    import math
    import numpy as np
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    run = str(tmp_path / 'run')
    assert T.main(['--norm', 'batch', '-f', '64', '--dataset', 'mnist', '--synthetic-size', '64', '-b', '16', '-e', '1', '--adjoint',
                   '--run-dir', run]) == 0
    ckpt = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ckpt['params']['norm'] == 'batch'
    assert math.isfinite(ckpt['metrics']['loss']) and ckpt['metrics']['nfe-f'] > 0 and ckpt['metrics']['nfe-b'] > 0
    assert 'odeblock.odefunc.norm1.weight' in ckpt['model'] and not any('running_mean' in k for k in ckpt['model'])
    E.main(['features', run])
    with np.load(os.path.join(run, 'features.npz')) as f:
        assert np.isfinite(f['features']).all() and f['features'].shape[-1] == 64

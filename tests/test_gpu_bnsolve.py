"""GPU: whole solves of the `norm='batch'` dynamics inside the library (bnsolve.py, csrc/bnsolve_api.hip: node_bnsolve_fwd /
node_bnsolve_adjoint), with `ODEfunc.batch_solve = True` unless said.  Cases, references and measures: tests/bnsolve_cases.py.

rk4 has no step decision, so its test is the sharp one for the layout, the time sign, the two multipliers (out_scale, da_scale),
the parameter offsets inside the adj_params segment, the adj_t seed and the hand-over between intervals: every shape x grid,
kink-free and ordinary parameters, against the fp64 oracle, with the bound  e_new <= 2 e_generic + e_floor  per quantity.
e_generic is the error of the same solve on the generic solver with the node (`batch_solve = False`), computed in the same
test; e_floor is what fp32 costs the oracle itself on the CPU (bnsolve_cases.E_FLOOR).  Both paths run the same kernels on the
same values and differ in rounding only: hence the factor two.

dopri5 runs are held to the project's own solver bounds (tests/test_gpu_bnfunc.py::test_generic_solver_on_the_node_against_the_oracle).

Measured on an MI355X, rk4, worst over the 25 cases, e_new / e_generic: outputs 1.31e-6 / 1.31e-6 ((2, 192, 7, 7), (0, 1), kink-free),
grad_y0 1.57e-6 / 1.57e-6 ((1, 64, 3, 3), (0, 1), ordinary), parameter gradients 2.20e-3 / 2.73e-3 ((64, 64, 8, 8)) and 8.0e-4 / 8.0e-4 over
the four small shapes.
(84, 64, 7, 7), (0, 1) -- chunks of 64 rows, the last of 20: second trips of the passes' row loops -- e_new / e_generic, ordinary:
outputs 5.6e-7 / 5.6e-7, grad_y0 4.7e-7 / 4.8e-7, parameter gradients 3.10e-3 / 3.02e-3; kink-free: 7.6e-7 / 7.6e-7, 6.0e-8 / 6.9e-8,
7.3e-4 / 6.8e-4.  Both sides of that bound run the same BatchNorm passes: a defect of the passes themselves is
tests/test_gpu_bnfunc.py's to find, what is held here is what a solve adds to them (out_scale, da_scale, the stage slots).
"""
import math
import os
from unittest import mock

import pytest
import torch

from tests import bnfunc_cases as B
from tests import bnsolve_cases as S

pytestmark = pytest.mark.gpu


def _func(C, kink_free=False, batch_solve=True):
    func, _ = B.func_pair(C, S.SEED, kink_free)
    func = func.cuda()
    func.batch_solve = batch_solve
    return func


def _run(func, shape, grid, method, tol=1e-3, batch_solve=True):
    import neural_ode_features_amd as nof
    func.batch_solve = batch_solve
    y, wgt = S.inputs(shape, grid)
    return S.solve(func, 'cuda', nof.odeint_adjoint, y, grid, tol, wgt, method)


def _check_rk4(shape, grid, kink_free):
    func = _func(shape[1], kink_free)
    ref = S.reference(shape, grid, kink_free, 'rk4')
    with mock.patch.object(_bnsolve()._BnOdeint, 'apply', wraps=_bnsolve()._BnOdeint.apply) as spy:
        new = _run(func, shape, grid, 'rk4')
    assert spy.call_count == 1
    gen = _run(func, shape, grid, 'rk4', batch_solve=False)
    assert torch.equal(new['out'][0], S.inputs(shape, grid)[0])
    n = len(grid) - 1
    assert new['nfe'] == gen['nfe'] == ref['nfe'] == (4 * n, 9 * n), (new['nfe'], gen['nfe'], ref['nfe'])
    e_new, e_gen = S.errors(new, ref), S.errors(gen, ref)
    bad = {}
    for k in ('out', 'gy', 'gp'):
        bound = 2 * e_gen[k] + S.E_FLOOR[k]
        print('%s %s %s: %-3s e_new %.2e  e_generic %.2e  bound %.2e' % (S.shape_id(shape), S.grid_id(grid), 'kinkfree' if kink_free else 'ordinary',
                                                                         k, e_new[k], e_gen[k], bound))
        if not e_new[k] <= bound:
            bad[k] = (e_new[k], e_gen[k], bound)
    assert not bad, bad


def _bnsolve():
    from neural_ode_features_amd import bnsolve
    return bnsolve


@pytest.mark.parametrize('kink_free', [False, True], ids=['ordinary', 'kinkfree'])
@pytest.mark.parametrize('grid', S.GRIDS, ids=S.grid_id)
@pytest.mark.parametrize('shape', S.SHAPES, ids=S.shape_id)
def test_rk4_against_the_fp64_oracle(shape, grid, kink_free):
    _check_rk4(shape, grid, kink_free)


def test_rk4_with_a_split_k_weight_gradient():
    _check_rk4(S.SPLITK_SHAPE, S.GRIDS[0], False)


@pytest.mark.parametrize('kink_free', [False, True], ids=['ordinary', 'kinkfree'])
def test_rk4_with_second_trips_of_the_row_loops(kink_free):
    """Chunks of 64 rows, the last one of 20 (tests/test_bnsolve_host.py asserts it): out_scale, da_scale and the writes into the
    stage-derivative slots in the second trip of every pass.  The oracle's own fp32 parameter gradients are 6.0e-3 (ordinary) and
    1.0e-3 (kink-free) off its fp64 ones at this shape, the former above E_FLOOR: the bound is relative to the generic solver, as
    for SPLITK_SHAPE."""
    _check_rk4(S.MULTIROW_SHAPE, S.GRIDS[0], kink_free)


def _same_nfe(hip, ref, intervals=1):
    """tests/test_gpu_bnfunc.py::_same_nfe: equal counters, or one accept / reject decision apart per solve."""
    (hf, hb), (rf, rb) = hip, ref
    df, db = abs(hf - rf), abs((hb - hf) - (rb - rf))
    return df % 6 == 0 and df <= 6 and db % 6 == 0 and db <= 6 * intervals


@pytest.mark.parametrize('grid', S.GRIDS, ids=S.grid_id)
def test_dopri5_against_the_oracle_and_the_generic_solver(grid):
    shape, tol = S.SHAPES[0], 1e-3
    func = _func(shape[1])
    ref = S.reference(shape, grid, False, 'dopri5', torch.float32)
    new = _run(func, shape, grid, 'dopri5')
    gen = _run(func, shape, grid, 'dopri5', batch_solve=False)
    n = len(grid) - 1
    print('%s: NFE new %s generic %s oracle %s; steps new %s generic %s' % (S.grid_id(grid), new['nfe'], gen['nfe'], ref['nfe'],
                                                                            (new['fwd'], new['bwd']), (gen['fwd'], gen['bwd'])))
    assert torch.equal(new['out'][0], S.inputs(shape, grid)[0])
    assert float((new['out'] - ref['out']).abs().max()) <= 10 * tol
    assert _same_nfe(new['nfe'], ref['nfe'], n), (new['nfe'], ref['nfe'])
    assert S.rel(new['gy'], ref['gy']) < 2e-2
    assert S.param_errors(new['gp'], ref['gp']) < 2e-2
    # stats: nfe is what the function's counter moved by
    assert new['fwd']['nfe'] == new['nfe'][0] == 2 + 6 * (new['fwd']['accepted'] + new['fwd']['rejected'])
    assert new['bwd']['nfe'] == new['nfe'][1] - new['nfe'][0] == 3 * n + 6 * (new['bwd']['accepted'] + new['bwd']['rejected'])
    assert new['fwd']['status'] == new['bwd']['status'] == 0 and new['fwd']['first_dt'] > 0
    assert new['fwd']['t_final'] >= (grid[-1] if grid[-1] > grid[0] else -grid[-1]) - 1e-6      # solver orientation
    # against the generic solver on the node
    assert abs(new['fwd']['accepted'] - gen['fwd']['accepted']) <= 1 and abs(new['bwd']['accepted'] - gen['bwd']['accepted']) <= n
    assert float((new['out'] - gen['out']).abs().max()) <= 10 * tol


def test_odeblock_last_only_and_its_gradient():
    """`solve_last` (what ODEBlock runs with return_last_only) returns the bits of out[-1] of the full call, and the gradient of
    the one slice equals the gradient of a zero-padded grad_out."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import integrate
    shape, grid = S.SHAPES[0], S.GRIDS[1]
    func = _func(shape[1])
    y, wgt = S.inputs(shape, grid)
    t = torch.tensor(grid).cuda()
    g_last = wgt[-1].cuda()

    def grads(last_only):
        for p in func.parameters():
            p.grad = None
        y0 = y.clone().cuda().requires_grad_(True)
        if last_only:
            out = integrate.solve_last(func, y0, t, 1e-3, 1e-3, 'dopri5', adjoint=True)
            assert out.shape == y0.shape
            out.backward(g_last)
            last = out
        else:
            out = nof.odeint_adjoint(func, y0, t, rtol=1e-3, atol=1e-3, method='dopri5')
            full = torch.zeros_like(out)
            full[-1] = g_last
            out.backward(full)
            last = out[-1]
        return last.detach().clone(), y0.grad.clone(), [p.grad.clone() for p in func.parameters()]

    a, b = grads(True), grads(False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    assert func.last_backward_stats['status'] == 0
    # the module path: an ODEBlock whose function has the switch
    blk = nof.ODEBlock(64, tol=1e-3, adjoint=True, norm='batch').cuda()
    blk.odefunc.batch_solve = True
    with mock.patch.object(_bnsolve()._BnOdeint, 'apply', wraps=_bnsolve()._BnOdeint.apply) as spy:
        out = blk(y.cuda().requires_grad_(True))
        out.sum().backward()
    assert spy.call_count == 1 and out.shape == tuple(shape) and blk.nfe > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in blk.parameters())


def test_cold_and_warm_solves_give_the_same_bits():
    """The first solve of a problem runs with hint 1 and several read-backs, the second with the learned hint (steps enqueued
    past the end of an interval run on discarded states): nothing may depend on the hint.  No atomics: two more repetitions
    give the same bits again."""
    bnsolve = _bnsolve()
    shape, grid = S.SHAPES[0], S.GRIDS[1]
    func = _func(shape[1])
    bnsolve._HINT.clear()
    runs = []
    hints = []
    for _ in range(4):
        runs.append(_run(func, shape, grid, 'dopri5'))
        hints.append(dict(bnsolve._HINT))
    assert len(hints[0]) == 2 and all(h == hints[0] for h in hints), hints
    for k in bnsolve._HINT:                      # far more steps than any interval needs: all but the first few run past the end
        bnsolve._HINT[k] = 12
    runs.append(_run(func, shape, grid, 'dopri5'))
    first = runs[0]
    for r in runs[1:]:
        assert torch.equal(r['out'], first['out']) and torch.equal(r['gy'], first['gy'])
        assert all(torch.equal(p, q) for p, q in zip(r['gp'], first['gp']))
        assert r['fwd'] == first['fwd'] and r['bwd'] == first['bwd'] and r['nfe'] == first['nfe']


LIBRARY_OPS = ('convolution', 'miopen', 'batch_norm', 'cat', 'relu', 'mul', 'copy_', 'transpose')


def _library_op(key):
    """An operator of PyTorch's that the solve must not dispatch: matched on the operator's own name (`aten::mul_` -> `mul_`),
    so that `AccumulateGrad` is not taken for a multiplication."""
    if '_BnOdeint' in key or '::' not in key:
        return False
    ns, op = key.lower().rsplit('::', 1)
    return ns.endswith('aten') and any(s in op for s in LIBRARY_OPS)


def test_dispatch_no_python_evaluation_and_no_library_operation():
    """With the switch: `bnfunc.evaluate` is never called and PyTorch dispatches no convolution, batch norm, concatenation, ReLU,
    multiplication or copy between the solve's first and last kernel (allocation is allowed; the list and the filter follow
    tests/test_gpu_bnfunc.py::test_node_runs_no_library_operation).  Class default: the generic solver on the node.  fused_batch
    off: the generic solver on the module operations."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import bnfunc
    from torch.profiler import ProfilerActivity, profile
    shape, grid = S.SHAPES[0], S.GRIDS[0]
    func = _func(shape[1])
    y, _ = S.inputs(shape, grid)
    t = torch.tensor(grid).cuda()

    def fwd_bwd(y0, cot, prof=None):
        out = nof.odeint_adjoint(func, y0, t, rtol=1e-3, atol=1e-3, method='dopri5')
        out.backward(cot)
        torch.cuda.synchronize()

    y0 = y.cuda().requires_grad_(True)
    cot = torch.ones((len(grid),) + tuple(shape), device='cuda')
    fwd_bwd(y0, cot)                              # warm: workspaces, the learned hint
    with mock.patch.object(bnfunc, 'evaluate', wraps=bnfunc.evaluate) as node:
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            fwd_bwd(y0, cot)
    assert node.call_count == 0
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if _library_op(k)]
    assert not bad, bad
    assert any('_BnOdeint' in k for k in names), names
    # the class default: the generic solver, every evaluation the node
    assert nof.ODEfunc.batch_solve is False
    plain, _ = B.func_pair(shape[1], S.SEED)
    plain = plain.cuda()
    with mock.patch.object(bnfunc, 'evaluate', wraps=bnfunc.evaluate) as node, \
            mock.patch.object(_bnsolve()._BnOdeint, 'apply', wraps=_bnsolve()._BnOdeint.apply) as spy:
        out = nof.odeint_adjoint(plain, y.cuda().requires_grad_(True), t, rtol=1e-3, atol=1e-3, method='dopri5')
        out.backward(cot)
    assert spy.call_count == 0 and node.call_count >= plain.nfe > 0
    # fused_batch off: the module operations under the generic solver, switch or not
    try:
        nof.ODEfunc.fused_batch = False
        with mock.patch.object(bnfunc, 'evaluate', wraps=bnfunc.evaluate) as node, \
                mock.patch.object(_bnsolve()._BnOdeint, 'apply', wraps=_bnsolve()._BnOdeint.apply) as spy:
            out = nof.odeint_adjoint(func, y.cuda().requires_grad_(True), t, rtol=1e-3, atol=1e-3, method='dopri5')
            out.backward(cot)
        assert spy.call_count == 0 and node.call_count == 0 and func.nfe > 0
    finally:
        nof.ODEfunc.fused_batch = True


@pytest.mark.parametrize('C', [16, 96])
def test_channels_the_kernels_refuse_run_the_generic_solver(C):
    import neural_ode_features_amd as nof
    func = _func(C)
    y = torch.randn(2, C, 6, 6, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    with mock.patch.object(_bnsolve()._BnOdeint, 'apply', wraps=_bnsolve()._BnOdeint.apply) as spy:
        out = nof.odeint_adjoint(func, y, torch.tensor([0.0, 1.0]).cuda(), rtol=1e-3, atol=1e-3, method='dopri5')
        out.sum().backward()
    assert spy.call_count == 0 and torch.isfinite(out).all() and torch.isfinite(y.grad).all()
    assert type(out.grad_fn).__name__ == '_GenericOdeintBackward'


def test_options_and_cpu_tensors_take_the_paths_they_take_today():
    import neural_ode_features_amd as nof
    func = _func(64)
    y = torch.randn(2, 64, 6, 6).cuda()
    t = torch.tensor([0.0, 1.0]).cuda()
    with pytest.raises(NotImplementedError):
        nof.odeint_adjoint(func, y, t, rtol=1e-3, atol=1e-3, method='dopri5', options={'record_dt': 8})
    with pytest.raises(RuntimeError):
        nof.odeint_adjoint(func, y.cpu(), t.cpu(), rtol=1e-3, atol=1e-3, method='dopri5')


def test_max_num_steps_raises_and_the_next_solve_is_correct():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import _lib
    shape, grid = S.SHAPES[0], S.GRIDS[0]
    func = _func(shape[1])
    y, _ = S.inputs(shape, grid)
    t = torch.tensor(grid).cuda()
    with pytest.raises(_lib.NodeHipError) as err:
        nof.odeint_adjoint(func, y.cuda(), t, rtol=1e-6, atol=1e-6, method='dopri5', options={'max_num_steps': 1})
    assert err.value.code == -5 and 'max_num_steps' in str(err.value)
    ref = S.reference(shape, grid, False, 'dopri5', torch.float32)
    new = _run(func, shape, grid, 'dopri5')
    assert float((new['out'] - ref['out']).abs().max()) <= 10 * 1e-3
    assert S.rel(new['gy'], ref['gy']) < 2e-2 and S.param_errors(new['gp'], ref['gp']) < 2e-2


def test_command_lines_train_and_features_use_the_batch_solve(tmp_path):
    """`train --norm batch` runs with `_BnOdeint` in the graph; `evaluate features` on the run writes finite features for all
    21 x 6 (t1, tol) pairs."""
    import numpy as np
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    run = str(tmp_path / 'run')
    bnsolve = _bnsolve()
    with mock.patch.object(bnsolve._BnOdeint, 'apply', wraps=bnsolve._BnOdeint.apply) as spy:
        assert T.main(['--norm', 'batch', '-f', '64', '--dataset', 'mnist', '--synthetic-size', '64', '-b', '16', '-e', '1', '-a',
                       '--run-dir', run]) == 0
    assert spy.call_count >= 4                       # one solve per batch
    ckpt = torch.load(os.path.join(run, 'last.pth'), map_location='cpu', weights_only=False)
    assert ckpt['params']['norm'] == 'batch' and math.isfinite(ckpt['metrics']['loss'])
    assert ckpt['metrics']['nfe-f'] > 0 and ckpt['metrics']['nfe-b'] > 0
    with mock.patch.object(bnsolve._BnOdeint, 'apply', wraps=bnsolve._BnOdeint.apply) as spy:
        E.main(['features', run])
    assert spy.call_count >= 6                       # one solve per tolerance and batch, 21 time points each
    with np.load(os.path.join(run, 'features.npz')) as f:
        feats = f['features']                        # [tols, t1s, N, C]
        assert np.isfinite(feats).all() and feats.shape[-1] == 64 and feats.shape[:2] == (6, 21), feats.shape

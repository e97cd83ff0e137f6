"""GPU parity of the adjoint's TIME gradients, and of the adjoint on multi-interval and reversed grids.

`node_solve_adjoint` returns grad_t [n_t] in upstream's `time_vjps` order: grad_t[0] is the integrated adj_time (the scalar segment
of the fused augmented solve: `Ctrl::ts_cur` through every stage, carried across intervals by launch_set_interval, dense output at
each interval's end), grad_t[i] = <f(t_i, y_i), dL/dy_i> for i >= 1 (k_dot_partial / k_dot_final with their sign, the `dots`
scratch, launch_copy_scalar_out).  The autograd surface discards it, so these tests call integrate.solve_forward and
integrate.solve_adjoint(..., want_grad_t=True) directly; the reference is the oracle's odeint_adjoint with a time grid that requires
grad (pinned on the CPU by tests/test_oracle_pinned.py::test_adjoint_time_gradient_vs_central_differences).

Every tight comparison is a REPLAY (tests.helpers.AT_FWD_DTS / AT_BWD_DTS in both directions): no accept / reject decision can
differ between the two sides, and no step lands on a target, so y, adj_y, adj_params and the scalar are dense-output at every
interval's end.  Parameters are kink-free.  The cotangent is aligned with f(t_i, y_i) (tests.helpers.adjoint_time_case): each
grad_t entry is then at least 5 % of sum ||f_j|| ||g_j|| (asserted: AT_MIN_COND) and a relative bound on it means something.

Cases: the smallest shape of each kernel family an adjoint solve can take (tests.helpers.AT_FAMILIES, each confirmed through
node_describe_dims), on the grids [0, 0.3, 0.55, 1], [1, 0.4, 0], [1, 0.25], [0, 1] (the pipeline shapes on the first two).

Bounds.  `out` (every slice), grad_y0 and grad_params: rel_err against the fp64 arbiter at the bounds the project already holds the
same quantities to -- 1e-5 / 2e-5 (test_gpu_solve.py::test_adjoint_replay_mode_tight) on the fp32 families, OUT_TOL / GRAD_TOL of
test_gpu_wide_pairs.py on the pipeline.  grad_t: max_i |got_i - ref_i| / max_i |ref_i| against the fp64 arbiter, at 8 x the largest
d32 of the family, rounded up to one significant digit, where d32 is the same error of the fp32 CPU ORACLE's replay (measured on
the CPU by tools/adjoint_time_d32.py; nothing of it comes from a kernel; tests.helpers.AT_GT_TOL holds the bounds, and
tests/test_adjoint_time_host.py checks the reference side without a GPU).  The factor: 4 for the pipeline's 22-bit operands against
fp32's 24, times 2 for a different summation order in a 512-partial fp32 dot.  d32 per case (profiles/adjoint_time_grads.txt):

    dopri5 replay                 [0,.3,.55,1]  [1,.4,0]   [1,.25]    [0,1]      max       bound
    small-C  (2, 16, 4, 4)        5.99e-07      8.01e-07   1.23e-07   8.38e-08   8.01e-07  7e-06
    fp32     (3, 32, 8, 8)        9.91e-07      3.30e-07   7.34e-08   6.37e-08   9.91e-07  8e-06
    w4-8x8   (8, 64, 8, 8)        2.23e-06      9.60e-07                         2.23e-06  2e-05
    w4-16x16 (2, 128, 16, 16)     3.84e-07      4.18e-08                         3.84e-07  4e-06
    rk4
    small-C  (2, 16, 4, 4)        8.39e-08      4.86e-08                         8.39e-08  7e-07
    fp32     (3, 32, 8, 8)        5.75e-08      1.55e-07                         1.55e-07  2e-06

NFE of a replayed adjoint solve: 2 (T - 1) + 6 steps.  Per interval api_solve.hip counts upstream's separate f(t_i, y_i)
(`S.nfe += 1`) and the interval's first evaluation (stage 0, the FSAL seed); the free-running law's third, the probe of the initial
step, is absent because a replay skips `initial_step`.  The oracle counts the same two (`stats.nfe += 1` in the backward loop,
`before_integrate`'s f0); the two counters are asserted equal.
"""
import os

import pytest
import torch

from tests.helpers import (AT_DOPRI5, AT_FAMILIES, AT_GT_TOL, AT_MIN_COND, AT_RK4, adjoint_time_case, at_err, at_hip_solve, at_id, rel_err)
from tests.test_gpu_wide_pairs import GRAD_TOL, OUT_TOL

pytestmark = pytest.mark.gpu

# out, gradients: test_gpu_solve.py::test_adjoint_replay_mode_tight and test_adjoint_rk4 hold them to these
FP32_OUT_TOL, FP32_GRAD_TOL = 1e-5, 2e-5
STATE_TOL = {'small-C': (FP32_OUT_TOL, FP32_GRAD_TOL), 'fp32': (FP32_OUT_TOL, FP32_GRAD_TOL),
             'w4-8x8': (OUT_TOL, GRAD_TOL), 'w4-16x16': (OUT_TOL, GRAD_TOL)}
GT_TOL = AT_GT_TOL      # grad_t: 8 x max d32 of the family, rounded up to one significant digit (the table above)


def _family(fam):
    """The family's shape, after node_describe_dims has confirmed what it selects."""
    from neural_ode_features_amd import _lib
    shape, want = AT_FAMILIES[fam]
    d = _lib.describe_dims(*shape)
    print('  %s %s selects' % (fam, shape), {k: d[k] for k in ('wgrad_kernel', 'conv_kernel', 'wino4', 'w4q', 'tiny', 'small', 'nsplit')})
    assert all(d[k] == v for k, v in want.items()), (fam, shape, want, d)
    return shape


def _steps(st):
    return st['accepted'] + st['rejected']


def _report(tag, fam, grid, method, mode, case, hip, ref, errs):
    """Print a case's figures; NODE_ADJOINT_TIME_TABLE=<file> also appends its row there (how profiles/adjoint_time_grads.txt is made)."""
    print('  %s: out %.2e  grad_y0 %.2e  grad_params %.2e  grad_t %.2e (bound %.0e, fp32 oracle d32 %s, min |grad_t| / sum |f||g| %.2f)'
          % (tag, errs['out'], errs['gy'], errs['gp'], errs['gt'], GT_TOL[(method, fam)],
             '%.2e' % case['d32'] if case['d32'] is not None else '-', case['cond']))
    print('    grad_t device %s\n    grad_t reference %s' % (hip['gt'].tolist(), ref['gt'].tolist()))
    path = os.environ.get('NODE_ADJOINT_TIME_TABLE')
    if path:
        with open(path, 'a') as fh:
            fh.write('%-44s d32 %.2e  bound %.0e  device grad_t %.2e  out %.2e  grad_y0 %.2e  grad_params %.2e\n'
                     % (at_id(fam, grid, method, mode), case['d32'], GT_TOL[(method, fam)], errs['gt'], errs['out'], errs['gy'], errs['gp']))


@pytest.mark.parametrize('fam,grid,method,mode', [pytest.param(*c, id=at_id(*c)) for c in AT_DOPRI5])
def test_adjoint_time_grads_replay_against_fp64(fam, grid, method, mode):
    """A replayed dopri5 adjoint solve against the fp64 arbiter's replay of the same steps: every output slice (forward dense output,
    also on decreasing grids), grad_y0, grad_params and grad_t, and the NFE law of both directions.  Bounds: the module docstring."""
    shape = _family(fam)
    case = adjoint_time_case(shape, grid, method, mode)
    hip, ref, o32 = at_hip_solve(case), case['f64'], case['o32']
    T = len(grid)
    if fam.startswith('w4'):
        print('  pair stats', hip['pair'])
    fs, bs = hip['fwd'], hip['bwd']
    print('  steps forward %d backward %d; nfe forward %d backward %d (oracle %d, %d)'
          % (_steps(fs), _steps(bs), fs['nfe'], bs['nfe'], o32['fwd'].nfe, o32['bwd'].nfe))
    assert fs['status'] == 0 and bs['status'] == 0
    assert fs['rejected'] == 0 and bs['rejected'] == 0
    assert (fs['accepted'], bs['accepted']) == (o32['fwd'].accepted, o32['bwd'].accepted)
    assert fs['nfe'] == 1 + 6 * fs['accepted'] == o32['fwd'].nfe
    assert bs['nfe'] == 2 * (T - 1) + 6 * bs['accepted'] == o32['bwd'].nfe
    errs = dict(out=rel_err(hip['out'], ref['out']), gy=rel_err(hip['gy'], ref['gy']), gp=rel_err(hip['gp'], ref['gp']),
                gt=at_err(hip['gt'], ref['gt']))
    _report('device vs fp64', fam, grid, method, mode, case, hip, ref, errs)
    assert hip['gt'].shape == (T,)
    assert case['cond'] >= AT_MIN_COND, case['cond']      # (the reference's grad_t is no cancelled sum)
    assert torch.equal(hip['out'][0], case['y'])
    out_tol, grad_tol = STATE_TOL[fam]
    assert errs['out'] < out_tol, errs
    assert errs['gy'] < grad_tol and errs['gp'] < grad_tol, errs
    assert errs['gt'] <= GT_TOL[(method, fam)], errs


@pytest.mark.parametrize('fam,grid,method,mode', [pytest.param(*c, id=at_id(*c)) for c in AT_RK4])
def test_adjoint_time_grads_rk4(fam, grid, method, mode):
    """rk4 (one 3/8-rule step per interval) over n_t = 4 and over a decreasing grid: out, grad_y0 and grad_params against the fp32
    CPU oracle at test_adjoint_rk4's bounds; grad_t against the fp64 arbiter like the replay cases (d32 is defined against it; the
    distance to the fp32 oracle is printed); nfe_b = 5 (T - 1)."""
    shape = _family(fam)
    case = adjoint_time_case(shape, grid, method, mode)
    hip, ref, o32 = at_hip_solve(case), case['f64'], case['o32']
    T = len(grid)
    assert hip['fwd']['nfe'] == 4 * (T - 1) == o32['fwd'].nfe
    assert hip['bwd']['nfe'] == 5 * (T - 1) == o32['bwd'].nfe
    errs = dict(out=rel_err(hip['out'], o32['out']), gy=rel_err(hip['gy'], o32['gy']), gp=rel_err(hip['gp'], o32['gp']),
                gt=at_err(hip['gt'], ref['gt']))
    _report('device vs fp32 oracle (grad_t vs fp64)', fam, grid, method, mode, case, hip, ref, errs)
    print('    grad_t device vs fp32 oracle %.2e' % at_err(hip['gt'], o32['gt']))
    assert errs['out'] < FP32_OUT_TOL and errs['gy'] < FP32_GRAD_TOL and errs['gp'] < FP32_GRAD_TOL, errs
    assert errs['gt'] <= GT_TOL[(method, fam)], errs


@pytest.mark.parametrize('fam', ['fp32', 'w4-8x8'])
def test_adjoint_time_grads_self_consistency(fam):
    """The library against itself (replay, n_t = 3): grad_y0 and grad_params bit-identical whether grad_t is requested or NULL; the
    same call twice gives a bit-identical grad_t; with grad_last_only the interior entries are exactly 0.0 and grad_t[0],
    grad_t[-1], grad_y0, grad_params agree with the full call given explicit zero slices within the replay bounds."""
    shape = _family(fam)
    grid = (1.0, 0.4, 0.0)
    case = adjoint_time_case(shape, grid, 'dopri5', 'replay', arbiter=False)
    with_t = at_hip_solve(case)
    again = at_hip_solve(case)
    without = at_hip_solve(case, want_grad_t=False)
    assert without['gt'] is None
    assert torch.equal(with_t['gy'], without['gy']) and torch.equal(with_t['gp'], without['gp'])
    assert torch.equal(with_t['gt'], again['gt']), (with_t['gt'], again['gt'])
    g_zero = torch.zeros_like(case['g'])
    g_zero[-1] = case['g'][-1]
    full = at_hip_solve(case, grad_out=g_zero)
    last = at_hip_solve(case, grad_last_only=True, grad_out=case['g'][-1].contiguous())
    print('  grad_t full call with zero slices %s\n  grad_t grad_last_only             %s' % (full['gt'].tolist(), last['gt'].tolist()))
    assert last['gt'].shape == (3,) and float(last['gt'][1]) == 0.0
    assert float(full['gt'][1]) == 0.0           # (a zero slice: the full call's dot product is an exact zero too)
    _, grad_tol = STATE_TOL[fam]
    e_y, e_p = rel_err(last['gy'], full['gy']), rel_err(last['gp'], full['gp'])
    e_t = at_err(last['gt'][[0, 2]], full['gt'][[0, 2]])
    print('  grad_last_only vs full: grad_y0 %.2e grad_params %.2e grad_t[0], grad_t[-1] %.2e' % (e_y, e_p, e_t))
    assert float(full['gt'][0]) != 0.0 and float(full['gt'][2]) != 0.0
    assert e_y < grad_tol and e_p < grad_tol and e_t <= GT_TOL[('dopri5', fam)]


@pytest.mark.parametrize('grid', [(0.0, 0.3, 1.0), (1.0, 0.4, 0.0)], ids=['0_0.3_1', '1_0.4_0'])
def test_adjoint_time_grads_free_running(grid):
    """A smoke check of the unforced path, one per direction, against the fp32 oracle at tol 1e-3: the NFE law 3 (T - 1) + 6 steps;
    with the same accept / reject history on both sides grad_t, grad_y0 and grad_params within 1e-3, otherwise only `out` within
    10 tol.  The replay cases carry the proof."""
    from tests.helpers import AT_TOL
    shape = _family('fp32')
    case = adjoint_time_case(shape, grid, 'dopri5', 'free', arbiter=False)
    hip, o32 = at_hip_solve(case), case['o32']
    T = len(grid)
    fs, bs = hip['fwd'], hip['bwd']
    same = ((fs['accepted'], fs['rejected'], bs['accepted'], bs['rejected']) ==
            (o32['fwd'].accepted, o32['fwd'].rejected, o32['bwd'].accepted, o32['bwd'].rejected))
    print('  device forward %s backward %s; oracle forward %s backward %s; same history %s'
          % ((fs['accepted'], fs['rejected']), (bs['accepted'], bs['rejected']), (o32['fwd'].accepted, o32['fwd'].rejected),
             (o32['bwd'].accepted, o32['bwd'].rejected), same))
    assert fs['nfe'] == 2 + 6 * _steps(fs)
    assert bs['nfe'] == 3 * (T - 1) + 6 * _steps(bs)
    e_out = float((hip['out'] - o32['out']).abs().max())
    errs = dict(gy=rel_err(hip['gy'], o32['gy']), gp=rel_err(hip['gp'], o32['gp']), gt=at_err(hip['gt'], o32['gt']))
    print('  max |out - oracle| %.2e; grad_y0 %.2e grad_params %.2e grad_t %.2e' % (e_out, errs['gy'], errs['gp'], errs['gt']))
    assert e_out <= 10 * AT_TOL
    if same:
        assert errs['gy'] < 1e-3 and errs['gp'] < 1e-3 and errs['gt'] < 1e-3, errs

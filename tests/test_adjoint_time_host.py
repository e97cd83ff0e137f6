"""What tests/test_gpu_adjoint_time.py stands on, checked without a GPU on its smallest shape: the aligned cotangent of
tests.helpers.adjoint_time_case makes every entry of the reference's grad_t a real gradient and not a cancelled sum, the fp32 CPU
oracle's own distance from the fp64 arbiter (d32) lies inside the bound derived from it, and the replay lists end every interval in
dense output (no step lands on a time point).  No kernel of the package runs here."""
import itertools

import pytest
import torch

from tests.helpers import (AT_BWD_DTS, AT_DOPRI5, AT_FAMILIES, AT_FWD_DTS, AT_GRIDS, AT_GT_TOL, AT_MIN_COND, AT_RK4, adjoint_time_case)


@pytest.mark.parametrize('grid,method,mode', [((0.0, 0.3, 0.55, 1.0), 'dopri5', 'replay'), ((1.0, 0.4, 0.0), 'rk4', 'fixed')])
def test_reference_time_gradient_is_well_conditioned_and_d32_inside_the_bound(grid, method, mode):
    shape = AT_FAMILIES['small-C'][0]
    case = adjoint_time_case(shape, grid, method, mode)
    T = len(grid)
    gt = case['f64']['gt']
    print('grad_t fp64 %s fp32 oracle %s  d32 %.2e  cond %.3f' % (gt.tolist(), case['o32']['gt'].tolist(), case['d32'], case['cond']))
    assert gt.shape == (T,) and case['o32']['gt'].shape == (T,) and case['g'].shape == (T,) + shape
    assert case['cond'] >= AT_MIN_COND
    assert case['d32'] <= AT_GT_TOL[(method, 'small-C')]
    assert case['times'] == [float(torch.tensor(v, dtype=torch.float32)) for v in grid]
    if method == 'dopri5':      # the oracle's counters: 1 + 6 steps forward, 2 per interval + 6 steps backward, nothing rejected
        fs, bs = case['o32']['fwd'], case['o32']['bwd']
        assert fs.rejected == 0 and bs.rejected == 0
        assert fs.nfe == 1 + 6 * fs.accepted and bs.nfe == 2 * (T - 1) + 6 * bs.accepted
    else:
        assert case['o32']['fwd'].nfe == 4 * (T - 1) and case['o32']['bwd'].nfe == 5 * (T - 1)


def test_no_replayed_step_lands_on_a_time_point():
    """Forward: one list over the whole grid; backward: the list restarts at every interval.  The last entry repeats.  Every
    partial sum stays at least 1e-3 away from every time point it could reach, so each interval ends in dense output on both sides."""
    def ends(dts, length):
        t, out = 0.0, []
        for dt in itertools.chain(dts, itertools.repeat(dts[-1])):
            t += dt
            out.append(t)
            if t > length:
                return out

    for grid in AT_GRIDS:
        offs = [abs(v - grid[0]) for v in grid[1:]]
        for e in ends(AT_FWD_DTS, offs[-1]):
            assert all(abs(e - o) > 1e-3 for o in offs), (grid, e)
        for a, b in zip(grid[:-1], grid[1:]):
            for e in ends(AT_BWD_DTS, abs(b - a)):
                assert abs(e - abs(b - a)) > 1e-3, (grid, a, b, e)


def test_case_lists_cover_what_the_module_claims():
    fams = {c[0] for c in AT_DOPRI5}
    assert fams == set(AT_FAMILIES)
    assert {(c[0], c[1]) for c in AT_DOPRI5 if c[0] in ('small-C', 'fp32')} == {(f, g) for f in ('small-C', 'fp32') for g in AT_GRIDS}
    assert all((c[2], c[0]) in AT_GT_TOL for c in AT_DOPRI5 + AT_RK4)
    assert any(g[0] > g[-1] and len(g) > 2 for g in AT_GRIDS) and any(g[0] < g[-1] and len(g) > 3 for g in AT_GRIDS)

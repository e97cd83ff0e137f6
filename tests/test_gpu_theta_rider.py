"""GPU: the theta finalize that rides in the next evaluation's P2 launch (k_w4s_pass_rider, NODE_TUNE_THETA_RIDER).

The rider moves launches, not arithmetic: every sum of the finalize enters in the order of the stand-alone kernel, so every
comparison here is torch.equal between NODE_TUNE_THETA_RIDER=0 (every finalize its own launch) and =1 -- outputs, all three
gradients, step counts and NFE of a forward + adjoint dopri5 solve through integrate.solve_forward / solve_adjoint."""
import pytest
import torch

from tests.deferred_record import new_record, read_record
from tests.helpers import make_func, tune_env

pytestmark = pytest.mark.gpu

_FUNCS = {}
_REFS = {}


def _func(C):
    if C not in _FUNCS:
        _FUNCS[C] = make_func(C, seed=31, device='cuda')[0]
    return _FUNCS[C]


def _data(shape, times, scale):
    gen = torch.Generator().manual_seed(32 + shape[0] + shape[1])
    y = scale * torch.randn(*shape, generator=gen)
    g = torch.randn(len(times), *shape, generator=gen) / (shape[1] * shape[2] * shape[3]) ** 0.5
    return y.cuda(), g.cuda()


def _solve(shape, tol, times, rider, env=None, scale=1.0, blind=None):
    """Forward + adjoint solve.  blind = (forward steps, backward steps): deferred completion with that many steps enqueued."""
    from neural_ode_features_amd import _lib, integrate
    f = _func(shape[1])
    rec = integrate.Recognised(f)
    mid = _lib.METHODS['dopri5']
    y, g = _data(shape, times, scale)
    res = {}
    with tune_env(NODE_TUNE_THETA_RIDER=rider, **(env or {})):
        bf = bb = None
        if blind is not None:
            recs = [new_record(), new_record()]
            flag = torch.zeros(1, dtype=torch.float32, device='cuda')
            bf, bb = (blind[0], recs[0], flag), (blind[1], recs[1], flag)
        out, fs = integrate.solve_forward(rec, rec.params, y, times, tol, tol, mid, None, blind=bf)
        gy, gp, gt, bs = integrate.solve_adjoint(rec, rec.params, out, g, times, tol, tol, mid, None, want_grad_t=True, blind=bb)
        torch.cuda.synchronize()
        if blind is not None:
            res['rec_fwd'], res['rec_bwd'], res['flag'] = read_record(recs[0]), read_record(recs[1]), float(flag)
    res.update(out=out, gy=gy, gp=gp, gt=gt, fwd=fs, bwd=bs)
    return res


def _same(a, b, stats=True):
    for k in ('out', 'gy', 'gp', 'gt'):
        assert torch.equal(a[k], b[k]), k
    assert bool(torch.isfinite(a['gp']).all()) and bool(torch.isfinite(a['gt']).all())
    if stats:
        for k in ('fwd', 'bwd'):
            for s in ('accepted', 'rejected', 'nfe'):
                assert a[k][s] == b[k][s], (k, s, a[k][s], b[k][s])


# (shape, environment): pairs with the 128-thread rider; the fp32 dU path; Q = 4 with the 256-thread rider; Q = 4 with cpg = 32
# (512-thread workgroups: the finalize stays a launch of its own whatever the switch says -- C = 1024, the selector takes N = 1)
SHAPES = [((16, 128, 8, 8), None), ((8, 128, 8, 8), {'NODE_TUNE_W4_F16': '0'}), ((4, 128, 16, 16), None), ((1, 1024, 16, 16), None)]


@pytest.mark.parametrize('shape,env', SHAPES, ids=['16x128x8x8', '8x128x8x8-f32', '4x128x16x16', '1x1024x16x16-cpg32'])
def test_rider_on_equals_rider_off(shape, env):
    off = _solve(shape, 1e-3, [0.0, 1.0], 0, env)
    on = _solve(shape, 1e-3, [0.0, 1.0], 1, env)
    print(shape, 'forward', (off['fwd']['accepted'], off['fwd']['rejected']), 'backward', (off['bwd']['accepted'], off['bwd']['rejected']))
    _same(off, on)
    assert off['bwd']['accepted'] >= 1 and float(off['gp'].abs().max()) > 0.0


def test_rider_tight_tolerance_with_rejected_steps():
    """tol 1e-5 on a state eight times the unit normal: more steps, and rejected ones -- a rejected step's stage derivatives are
    overwritten by the repeated step's, riders included."""
    off = _solve((16, 128, 8, 8), 1e-5, [0.0, 1.0], 0, scale=8.0)
    on = _solve((16, 128, 8, 8), 1e-5, [0.0, 1.0], 1, scale=8.0)
    print('tol 1e-5: forward', (off['fwd']['accepted'], off['fwd']['rejected']), 'backward', (off['bwd']['accepted'], off['bwd']['rejected']))
    assert off['bwd']['rejected'] > 0
    _same(off, on)


def test_rider_two_interval_grid():
    off = _solve((16, 128, 8, 8), 1e-3, [0.0, 0.4, 1.0], 0)
    on = _solve((16, 128, 8, 8), 1e-3, [0.0, 0.4, 1.0], 1)
    _same(off, on)
    assert off['gt'].numel() == 3


def test_rider_blocks_honour_done_in_a_spare_step():
    """A deferred solve with one spare step enqueued against the exact count: the spare step's launches -- four of them P2
    launches with a rider -- must do nothing once the interval is over (Ctrl::done)."""
    shape, times = (16, 128, 8, 8), [0.0, 1.0]
    sync = _solve(shape, 1e-3, times, 1)
    nf = sync['fwd']['accepted'] + sync['fwd']['rejected']
    nb = sync['bwd']['accepted'] + sync['bwd']['rejected']
    exact = _solve(shape, 1e-3, times, 1, blind=(nf, nb))
    spare = _solve(shape, 1e-3, times, 1, blind=(nf + 1, nb + 1))
    spare2 = _solve(shape, 1e-3, times, 1, blind=(nf + 2, nb + 2))
    off = _solve(shape, 1e-3, times, 0, blind=(nf + 1, nb + 1))
    for r in (exact, spare, spare2, off):
        assert r['flag'] == 0.0 and r['rec_fwd']['miss'] == 0 and r['rec_bwd']['miss'] == 0
        assert r['rec_fwd']['steps'] == nf and r['rec_bwd']['steps'] == nb and r['rec_bwd']['done'] == 1
        _same(sync, r, stats=False)


def test_rider_time_gradient_is_the_same_over_repeated_solves():
    """The fence-free arrival counter of the finalize under the rider's block shape: twenty solves, one grad_t."""
    first = _solve((16, 128, 8, 8), 1e-3, [0.0, 1.0], 1)
    for _ in range(19):
        again = _solve((16, 128, 8, 8), 1e-3, [0.0, 1.0], 1)
        assert torch.equal(first['gt'], again['gt']) and torch.equal(first['gp'], again['gp'])

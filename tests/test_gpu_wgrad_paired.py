"""GPU: an augmented evaluation's weight gradient and conv-1 data gradient as ONE launch (k_w4_gemm64h_wgrad64h,
NODE_TUNE_WGRAD_PAIRED).

The paired kernel runs the two stand-alone kernels' bodies on a concatenated grid: every sum enters in the same order, so every
comparison is np.array_equal between NODE_TUNE_WGRAD_PAIRED=0 (two launches) and a paired variant -- the state gradient, the
parameter gradient, the time gradient and the step records of a forward + adjoint dopri5 solve at tol 1e-3 through
integrate.solve_forward / solve_adjoint.  The library re-reads the switch on every call, so both settings run in one process.
Variants: 1 the weight gradient's workgroups first (256 registers; the default), 3 the GEMM's first, 5 the GEMM's own register budget."""
import numpy as np
import pytest
import torch

from tests.deferred_record import new_record, read_record
from tests.helpers import make_func, tune_env

pytestmark = pytest.mark.gpu

_FUNCS = {}
_OFF = {}
TOL, TIMES = 1e-3, [0.0, 1.0]


def _func(C):
    if C not in _FUNCS:
        _FUNCS[C] = make_func(C, seed=41, device='cuda')[0]
    return _FUNCS[C]


def _solve(shape, paired, blind=None, profile=False):
    """Forward + adjoint solve.  blind = (forward steps, backward steps): deferred completion with that many steps enqueued."""
    from neural_ode_features_amd import _lib, integrate
    rec = integrate.Recognised(_func(shape[1]))
    mid = _lib.METHODS['dopri5']
    gen = torch.Generator().manual_seed(42 + shape[0] + shape[1])
    y = torch.randn(*shape, generator=gen).cuda()
    g = (torch.randn(len(TIMES), *shape, generator=gen) / (shape[1] * shape[2] * shape[3]) ** 0.5).cuda()
    res = {}
    with tune_env(NODE_TUNE_WGRAD_PAIRED=paired):
        bf = bb = None
        if blind is not None:
            recs = [new_record(), new_record()]
            flag = torch.zeros(1, dtype=torch.float32, device='cuda')
            bf, bb = (blind[0], recs[0], flag), (blind[1], recs[1], flag)
        out, fs = integrate.solve_forward(rec, rec.params, y, TIMES, TOL, TOL, mid, None, blind=bf)
        if profile:
            integrate.profile_begin()
        gy, gp, gt, bs = integrate.solve_adjoint(rec, rec.params, out, g, TIMES, TOL, TOL, mid, None, want_grad_t=True, blind=bb)
        torch.cuda.synchronize()
        if profile:
            res['prof'] = {k: v['launches'] for k, v in integrate.profile_end().items()}
        if blind is not None:
            res['rec_fwd'], res['rec_bwd'], res['flag'] = read_record(recs[0]), read_record(recs[1]), float(flag)
    res.update(out=out.cpu().numpy(), gy=gy.cpu().numpy(), gp=gp.cpu().numpy(), gt=gt.cpu().numpy(), fwd=fs, bwd=bs)
    return res


def _off(shape):
    """The two-launch solve of a shape, profiled: computed once and left unchanged.  (A first, unprofiled solve leaves the library its
    step count: the profiled ones then enqueue the same number of steps whatever the switch says.)"""
    if shape not in _OFF:
        first = _solve(shape, 0)
        _OFF[shape] = _solve(shape, 0, profile=True)
        _same(first, _OFF[shape])
    return _OFF[shape]


def _same(a, b, stats=True):
    for k in ('out', 'gy', 'gp', 'gt'):
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a['gp']).all() and np.isfinite(a['gt']).all()
    if stats:
        for k in ('fwd', 'bwd'):
            for s in ('accepted', 'rejected', 'nfe'):
                assert a[k][s] == b[k][s], (k, s, a[k][s], b[k][s])


# (shape, whether the solve takes the pair).  The first four: the smallest shape both kernels accept; row blocks not a power of two;
# C = 256; Q = 4.  Three of them have N Q = 16 rows of samples, which the solver's selector gives to k_w4_gemm_small (fp32 filters: a
# solve that never forms fp16 pairs, w4_select.hip) -- they hold the switch harmless there.  The last three are their neighbours at
# N Q = 32, the smallest batch whose adjoint solve runs on fp16 pairs: most workgroups of either half are edge cases; C = 256 (four
# weight-gradient tiles per pair, ring depth 4 in the stand-alone GEMM against 2 in the pair); Q = 4.
SHAPES = [((16, 128, 8, 8), False), ((48, 128, 8, 8), True), ((16, 256, 8, 8), False), ((4, 128, 16, 16), False),
          ((32, 128, 8, 8), True), ((32, 256, 8, 8), True), ((8, 128, 16, 16), True)]


@pytest.mark.parametrize('shape,takes_pair', SHAPES, ids=['x'.join(map(str, s)) for s, _ in SHAPES])
@pytest.mark.parametrize('variant', [1, 3, 5])
def test_paired_equals_two_launches(shape, takes_pair, variant):
    off = _off(shape)
    on = _solve(shape, variant, profile=True)
    print(shape, variant, 'backward', (off['bwd']['accepted'], off['bwd']['rejected']), 'weight gradients', off['prof']['wgrad_gemm'],
          'GEMM launches off / on', off['prof']['w4_component_gemm'], on['prof']['w4_component_gemm'])
    _same(off, on)
    assert off['bwd']['accepted'] >= 1 and float(np.abs(off['gp']).max()) > 0.0
    # the pair really ran: every weight-gradient launch but the interval's first evaluation (bf16 triples: the cotangent's fp16 scale is
    # not known yet) took its conv-1 GEMM along.  Class 1 counts the weight gradients (stand-alone or paired), class 2 the GEMMs
    w = off['prof']['wgrad_gemm']
    assert on['prof']['wgrad_gemm'] == w and w >= 2
    assert off['prof']['w4_component_gemm'] - on['prof']['w4_component_gemm'] == (w - 1 if takes_pair else 0)
    for k, v in off['prof'].items():
        if k not in ('wgrad_gemm', 'w4_component_gemm'):
            assert on['prof'][k] == v, k


def test_both_halves_honour_done_in_a_spare_step():
    """A deferred solve with one spare step enqueued against the exact count: the spare step's paired launches meet Ctrl::done
    set, and both halves must return without a store."""
    shape = (32, 128, 8, 8)
    sync = _off(shape)
    nf = sync['fwd']['accepted'] + sync['fwd']['rejected']
    nb = sync['bwd']['accepted'] + sync['bwd']['rejected']
    runs = [_solve(shape, 1, blind=(nf, nb)), _solve(shape, 1, blind=(nf + 1, nb + 1)), _solve(shape, 0, blind=(nf + 1, nb + 1)),
            _solve(shape, 3, blind=(nf + 1, nb + 1))]
    for r in runs:
        assert r['flag'] == 0.0 and r['rec_fwd']['miss'] == 0 and r['rec_bwd']['miss'] == 0
        assert r['rec_fwd']['steps'] == nf and r['rec_bwd']['steps'] == nb and r['rec_bwd']['done'] == 1
        _same(sync, r, stats=False)


# shapes the pair does not take: C = 64 (no 128 x 128 weight-gradient tile), N Q % 16 != 0 (no 64-row GEMM tile on fp16 pairs)
FALLBACKS = [(16, 64, 8, 8), (8, 128, 8, 8)]


@pytest.mark.parametrize('shape', FALLBACKS, ids=['x'.join(map(str, s)) for s in FALLBACKS])
def test_other_shapes_keep_two_launches(shape):
    off = _off(shape)
    on = _solve(shape, 1, profile=True)
    print(shape, 'weight gradients', off['prof']['wgrad_gemm'], 'GEMM launches off / on', off['prof']['w4_component_gemm'],
          on['prof']['w4_component_gemm'])
    assert on['prof'] == off['prof'] and off['prof']['wgrad_gemm'] >= 2
    _same(off, on)

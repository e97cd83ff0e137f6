"""The fp64 restatement of one flat-solver step (tests/helpers.py, sc_*) against oracle/torchdiffeq_restated.py in fp64, and the
input conditions tests/test_gpu_step_control.py relies on.  No device is needed.

The restatement uses the kernels' coefficients: every tableau entry rounded to fp32 before it is widened.  That rounding is the ONLY
difference to the oracle, which keeps the exact doubles: a coefficient c becomes c (1 + d) with |d| <= 2^-24, so a combination
dt * sum_j c_j k_j moves by at most 2^-24 * |dt| * sum_j |c_j| |k_j| per element.  Every bound below is that expression (pushed
through the formula where the combination is used further) plus 1e-13 relative for the fp64 arithmetic of both sides."""
import numpy as np
import pytest
import torch

from oracle import torchdiffeq_restated as tdq
from tests import helpers as H

U = 2.0 ** -24          # unit roundoff of fp32: the relative error of a coefficient rounded to fp32
EPS = 1e-13             # fp64 arithmetic of two orderings of the same short sums, relative to the largest entry
SIZES = {1: [1027], 2: [5, 1027], 3: [33, 7, 1]}       # tuple states of 1, 2, 3 tensors of unequal length
T0, DT = 0.25, 0.0625


def _state(nt, seed=0):
    rng = np.random.default_rng(seed + nt)
    ys = [rng.standard_normal(n).astype(np.float32) for n in SIZES[nt]]
    ks = [[rng.standard_normal(n).astype(np.float32) for _ in range(7)] for n in SIZES[nt]]
    return ys, ks


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _comb_bound(ks, coef, dt):
    return U * abs(dt) * sum(abs(float(c)) * np.abs(k.astype(np.float64)) for c, k in zip(coef, ks))


def _close(got, want, bound):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(np.abs(got - want) <= bound + EPS * (np.abs(want).max() + 1e-30)), float(np.max(np.abs(got - want) - bound))


class _Replay:
    """Dynamics that return recorded derivatives and remember where they were evaluated."""

    def __init__(self, outs):
        self.outs, self.calls = list(outs), []

    def __call__(self, t, y):
        self.calls.append((float(t), [v.numpy().copy() for v in y]))
        return self.outs[len(self.calls) - 1]


@pytest.mark.parametrize('nt', [1, 2, 3])
def test_dopri5_stages_and_error_estimate_match_runge_kutta_step(nt):
    ys, ks = _state(nt)
    fn = _Replay([tuple(_t(k[s + 1]) for k in ks) for s in range(6)])
    y1, f1, err, _ = tdq._runge_kutta_step(fn, tuple(_t(y) for y in ys), tuple(_t(k[0]) for k in ks), torch.tensor(T0, dtype=torch.float64),
                                           torch.tensor(DT, dtype=torch.float64))
    for s in range(6):
        t_or, y_or = fn.calls[s]
        for i in range(nt):
            st, ts = H.sc_stage(ys[i], ks[i], T0, DT, 1.0, s)
            _close(st, y_or[i], _comb_bound(ks[i], H.SC_BETA[s], DT))
            _close(ts, t_or, U * abs(DT) * float(H.SC_ALPHA[s]))
            assert float(H.sc_stage(ys[i], ks[i], T0, DT, -1.0, s)[1]) == -float(ts)
    for i in range(nt):           # the error estimate the ratio is built on, and c_sol == the sixth row (FSAL)
        e = H.sc_lincomb(np.zeros_like(ys[i]), ks[i], H.SC_CERR, DT)
        _close(e, err[i].numpy(), _comb_bound(ks[i], H.SC_CERR, DT))
        _close(H.sc_lincomb(ys[i], ks[i], H.SC_CSOL, DT), y1[i].numpy(), _comb_bound(ks[i], H.SC_CSOL, DT))
    assert H.sc_stage(ys[0], ks[0], T0, DT, 1.0, H.SC_F0) == (None, T0)


@pytest.mark.parametrize('nt', [1, 2, 3])
def test_error_ratio_and_step_size_match_the_oracle(nt):
    ys, ks = _state(nt, seed=10)
    y1s = [H.sc_stage(y, k, T0, DT, 1.0, 5)[0].astype(np.float32) for y, k in zip(ys, ks)]
    rtol, atol = 1e-3, 1e-4
    got, _, _ = H.sc_error_ratios(ys, y1s, ks, DT, rtol, atol)
    err = tuple(tdq._scaled_dot_product(torch.tensor(DT, dtype=torch.float64), tdq.DP_C_ERROR, [_t(a) for a in k]) for k in ks)
    want = tdq._compute_error_ratio(err, float(np.float32(rtol)), float(np.float32(atol)), tuple(_t(y) for y in ys), tuple(_t(y) for y in y1s))
    for i in range(nt):
        tol = float(np.float32(atol)) + float(np.float32(rtol)) * np.maximum(np.abs(ys[i]), np.abs(y1s[i])).astype(np.float64)
        b = _comb_bound(ks[i], H.SC_CERR, DT)
        e = np.abs(err[i].numpy())
        _close(got[i], float(want[i]), float(np.mean((2 * e * b + b * b) / tol ** 2)))
    # the scalar segment is a segment of one element
    sv, sk = np.float32(0.7), [np.float32(v) for v in np.random.default_rng(3).standard_normal(7)]
    r, _, s_new = H.sc_error_ratios([], [], [], DT, rtol, atol, scalar=(sv, sk))
    one = [np.array([v], dtype=np.float32) for v in sk]
    r1, _, _ = H.sc_error_ratios([np.array([sv])], [np.array([s_new])], [one], DT, rtol, atol)
    _close(s_new, H.sc_lincomb(np.array([sv]), one, H.SC_CSOL, DT)[0], 0.0)
    _close(r[0], r1[0], 0.0)
    # the step size from the oracle's own ratios: no coefficient involved, fp64 rounding only -- all three regimes
    for scale in (1.0, 0.0, 1e-3, 5.0, 1e4, 1e12):
        rat = tuple(w * scale for w in want)
        o = float(tdq._optimal_step_size(torch.tensor(DT, dtype=torch.float64), rat))
        mine, regime = H.sc_dt_next(DT, max(float(x) for x in rat))
        _close(mine, o, 0.0)
        big = max(float(x) for x in rat)
        assert regime == ('x10' if big == 0 else 'clamp' if (0.9 ** 10 <= big < 1 or big >= 4.5 ** 10 or big <= 0.09 ** 10) else 'free')
    d = H.sc_decide([0.5, 0.2], 1.0, 0.5, [1.2, 1.5, 1.7], 0)
    assert (d['accept'], d['t'], d['j0'], d['j1'], d['done']) == (True, 1.5, 0, 2, False)
    d = H.sc_decide([0.5, 1.5], 1.0, 0.5, [1.2], 0)
    assert (d['accept'], d['t'], d['j1'], d['done']) == (False, 1.0, 0, False)
    assert H.sc_decide([0.5], 1.0, 0.5, [1.2], 0)['done'] and H.sc_decide([float('nan')], 1.0, 0.5, [1.2])['status'] == H.SC_NONFINITE
    assert H.sc_decide([float('inf')], 1.0, 0.5, [1.2])['status'] == H.SC_NONFINITE


def _init_oracle(c):
    sc = c['scalar']
    y = tuple(_t(a) for a in c['y']) + (() if sc is None else (_t([sc[0]]),))
    f0 = tuple(_t(a) for a in c['f0']) + (() if sc is None else (_t([sc[1]]),))
    f1 = tuple(_t(a) for a in c['f1']) + (() if sc is None else (_t([sc[2]]),))
    fn = _Replay([f1])
    rtol, atol = (float(np.float32(v)) for v in H.SC_INIT_TOL)
    dt = tdq._select_initial_step(fn, torch.tensor(T0, dtype=torch.float64), y, 4, rtol, atol, f0)
    return float(dt), fn.calls[0]


def _init_mine(c, F=np.float64):
    sc = c['scalar']
    return H.sc_initial_step(c['y'], c['f0'], lambda h0: (c['f1'], None if sc is None else sc[2]), *H.SC_INIT_TOL,
                             scalar=None if sc is None else sc[:2], F=F)


@pytest.mark.parametrize('name', H.SC_INIT_CASES)
def test_initial_step_matches_select_initial_step(name):
    c = H.sc_init_case(name)
    dt_o, (t_probe, y_probe) = _init_oracle(c)
    m = _init_mine(c)
    _close(m['dt'], dt_o, 0.0)                      # no tableau coefficient here: fp64 rounding only
    _close(T0 + m['h0'], t_probe, 0.0)
    for i, y in enumerate(c['y']):
        _close(H.sc_stage(y, [c['f0'][i]], T0, DT, 1.0, H.SC_PROBE, h0=m['h0'])[0], y_probe[i], 0.0)
    # the branches and maxima the GPU cases are named after
    with np.errstate(all='ignore'):
        q = [a / b for a, b in zip(m['d0'], m['d1'])]
    if name == 'y_zero':
        assert max(m['d0']) == 0.0 and m['h0'] == H.SC_TINY_H and m['dt'] == 100 * H.SC_TINY_H
    elif name == 'f_zero':
        assert max(m['d1']) == 0.0 and max(m['d2']) == 0.0 and m['h0'] == H.SC_TINY_H and m['dt'] == H.SC_TINY_H
    else:
        assert min(max(m['d0']), max(m['d1'])) > 1e-3 and max(m['d2']) > 1e-9      # far from the 1e-5 / 1e-15 thresholds
        assert 100 * m['h0'] > 1.5 * m['dt'] or 100 * m['h0'] < m['dt'] / 1.5         # and from the tie of min(100 h0, h1)
    if name == 'seg3':
        assert [int(np.argmax(v)) for v in (q, m['d1'], m['d2'])] == [0, 1, 2]
    if name == 'scalar_max':
        assert [int(np.argmax(v)) for v in (m['d0'], q, m['d1'], m['d2'])] == [2, 2, 2, 2]
    if name == 'seg2_scalar':
        assert all(int(np.argmax(v)) < 2 for v in (q, m['d1'], m['d2']))


@pytest.mark.parametrize('nt', [1, 2, 3])
def test_dense_output_matches_interp_fit_and_evaluate(nt):
    ys, ks = _state(nt, seed=20)
    y1s = [H.sc_stage(y, k, T0, DT, 1.0, 5)[0].astype(np.float32) for y, k in zip(ys, ks)]
    dt = torch.tensor(DT, dtype=torch.float64)
    co = tdq._interp_fit_dopri5(tuple(_t(y) for y in ys), tuple(_t(y) for y in y1s), tuple([_t(a) for a in k] for k in ks), dt)
    for x in (0.0, 0.3, 0.77, 1.0):
        tt = T0 + x * DT if x < 1 else T0 + DT
        want = tdq._interp_evaluate(co, T0, T0 + DT, tt)
        xx = (tt - T0) / DT
        for i in range(nt):
            b = _comb_bound(ks[i], H.SC_CMID, DT) * (16 * xx ** 4 + 32 * xx ** 3 + 16 * xx ** 2)     # |d out / d y_mid| summed termwise
            _close(H.sc_dense(ys[i], y1s[i], ks[i], DT, T0, T0 + DT, tt), want[i].numpy(), b + 1e-12)


@pytest.mark.parametrize('nt', [1, 2, 3])
def test_rk4_stages_and_update_match_rk4_alt_step(nt):
    ys, ks = _state(nt, seed=30)
    fn = _Replay([tuple(_t(k[s]) for k in ks) for s in range(4)])
    dy = tdq._rk4_alt_step(fn, torch.tensor(T0, dtype=torch.float64), torch.tensor(DT, dtype=torch.float64), tuple(_t(y) for y in ys))
    for s in (1, 2, 3):
        t_or, y_or = fn.calls[s]
        for i in range(nt):
            st, ts = H.sc_stage(ys[i], ks[i], T0, DT, 1.0, s, method='rk4')
            _close(st, y_or[i], _comb_bound(ks[i], H.SC_RK4_ROWS[s - 1], DT))
            _close(ts, t_or, U * DT)
    for i in range(nt):
        _close(H.sc_rk4_finish(ys[i], ks[i], DT), ys[i].astype(np.float64) + dy[i].numpy(), 0.0)      # 1/8, 3/8: exact in fp32
    v, sk = np.float32(0.3), [k[0] for k in ks[0][:4]]
    _close(H.sc_rk4_finish_scalar(v, sk, DT), H.sc_rk4_finish(np.array([v]), [np.array([a]) for a in sk], DT)[0], 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# Input conditions of tests/test_gpu_step_control.py, shown on the reference alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def step_cases():
    return {name: H.sc_case(**kw) for name, kw, _ in H.SC_STEP_CASES}


def test_every_decision_case_lies_in_its_band_and_away_from_one(step_cases):
    devs = []
    for name, kw, band in H.SC_STEP_CASES:
        st = step_cases[name]
        r64, elems, _ = H.sc_error_ratios(st['y'], st['y1'], st['k'], st['dt'], st['rtol'], st['atol'], st['scalar'])
        lo, hi = H.SC_BANDS[band]
        big = max(float(r) for r in r64)
        assert lo <= big <= hi, (name, big)
        assert all(not (0.9 <= float(r) <= 1.1) for r in r64), (name, r64)          # no decision within 10 % of a ratio of 1
        d = H.sc_decide(r64, st['t'], st['dt'], [st['t'] + 10.0])
        assert d['accept'] == (band in ('free', 'clamp', 'zero')) and d['regime'] == {'free': 'free', 'reject': 'free', 'clamp': 'clamp',
                                                                                     'huge': 'clamp', 'zero': 'x10'}[band]
        if 'spike' in kw:
            sg, idx = kw['spike']
            assert elems[sg][idx] > 0.5 * elems[sg].sum(), name
        if name == 'seg3_last_rejects':
            assert r64[0] < 0.9 and r64[1] < 0.9 and r64[2] > 1.1
        if name == 'seg2_scalar_rejects':
            assert r64[0] < 0.9 and r64[1] < 0.9 and r64[2] > 1.1
        if name == 'seg3_middle_max':
            assert int(np.argmax(r64)) == 1 and abs(float(np.mean(r64)) / big - 1) > 0.1      # a mean over segments is far off
        # the same statement at the kernels' precision: how far correct fp32 arithmetic lies from fp64
        r32, _, s32 = H.sc_error_ratios(st['y'], st['y1'], st['k'], st['dt'], st['rtol'], st['atol'], st['scalar'], F=np.float32)
        devs += [abs(float(a) / float(b) - 1) for a, b in zip(r32, r64) if float(b) != 0]
    print('largest fp32 deviation of a mean ratio: %.3g' % max(devs))
    assert max(devs) <= H.SC_DEV_RATIO


def test_fp32_deviation_of_the_initial_step_is_what_the_gpu_tolerance_assumes():
    devs = []
    for name in H.SC_INIT_CASES:
        c = H.sc_init_case(name)
        a, b = _init_mine(c), _init_mine(c, F=np.float32)
        devs += [abs(b['h0'] / a['h0'] - 1), abs(b['dt'] / a['dt'] - 1)]
    print('largest fp32 deviation of h0 / dt: %.3g' % max(devs))
    assert max(devs) <= H.SC_DEV_INIT


def test_fp32_deviation_of_the_per_element_outputs_is_what_the_gpu_tolerance_assumes(step_cases):
    dev_stage, dev_dense = [], []
    for name in ('n5', 'n1027', 'sweep2', 'seg2_scalar', 'seg3_middle_max'):
        st = step_cases[name]
        for t0 in (0.0, st['t']):
            for i, (y, k) in enumerate(zip(st['y'], st['k'])):
                ymax = float(np.abs(y).max())
                for stage, method in [(s, 'dopri5') for s in range(6)] + [(s, 'rk4') for s in (1, 2, 3)]:
                    a, ta = H.sc_stage(y, k, t0, st['dt'], -1.0, stage, method)
                    b, tb = H.sc_stage(y, k, t0, st['dt'], -1.0, stage, method, F=np.float32)
                    dev_stage.append(float(np.abs(a - b).max()) / ymax)
                    dev_stage.append(abs(float(ta) - float(tb)) / max(abs(float(ta)), 1e-30))
                dev_stage.append(float(np.abs(H.sc_rk4_finish(y, k, st['dt']) - H.sc_rk4_finish(y, k, st['dt'], F=np.float32)).max()) / ymax)
                for x in (0.3, 0.5, 0.9, 1.0):
                    t1 = t0 + st['dt']
                    tt = t0 + x * st['dt'] if x < 1 else t1
                    a = H.sc_dense(y, st['y1'][i], k, st['dt'], t0, t1, tt)
                    b = H.sc_dense(y, st['y1'][i], k, st['dt'], t0, t1, tt, F=np.float32)
                    dev_dense.append(float(np.abs(a - b).max()) / ymax)
    print('largest fp32 deviation relative to max|y|: stage %.3g, dense output %.3g' % (max(dev_stage), max(dev_dense)))
    assert max(dev_stage) <= H.SC_DEV_STAGE and max(dev_dense) <= H.SC_DEV_DENSE


@pytest.mark.parametrize('n', H.SC_DENSE_SIZES)
def test_dense_output_scenario_passes_three_one_and_no_target(n):
    st, targets = H.sc_dense_scenario(n)
    j, passed = 0, []
    for _ in range(3):
        d = H.sc_finish_step(st, targets, j)
        assert d['accept'] and not d['done'] and all(0.0 < float(r) < 0.9 for r in d['ratios']), d['ratios']
        passed.append((d['j0'], d['j1']))
        if d['j1'] > d['j0']:        # no target within 1e-3 dt of a step's end unless it IS the end: the device's dt differs by ~1e-7
            assert all(tt == d['t'] or tt < d['t'] - 1e-3 * st['dt'] for tt in targets[d['j0']:d['j1']])
        assert targets[d['j1']] > d['t'] + 1e-3 * st['dt']
        j, st = d['j1'], H.sc_advance(st, d, d['dt_next'])
    assert passed == [(0, 3), (3, 4), (4, 4)] and targets[2] == 0.25 + 0.0625

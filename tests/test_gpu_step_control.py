"""The step-control kernels, each on its own, element by element against the fp64 restatement of tests/helpers.py (sc_*), which
tests/test_step_control_host.py pins to the oracle: k_lincomb, k_init_norms + k_init_controller, k_error_norm + k_step_controller,
k_emit_flat, k_commit, k_flat_scalar, k_flat_time, k_set_scalar_state -- driven through generic.FlatSolve (node_flat_*) on buffers
filled with chosen data.  No dynamics function, no convolution.

Sizes (csrc/kernels_step_control.hip; every kernel runs 256 threads per workgroup):
  * k_error_norm: grid ERR_BLOCKS = 512, one float4 per thread and sweep -> a sweep covers 512 * 256 * 4 = 524288 elements; the
    n % 4 tail is block 0's.  524288 + 5 = one float4 of a second sweep + a tail of one; 1027 = 256 float4 + a tail of three.
  * k_init_norms: grid 512, one ELEMENT per thread and sweep -> 131072 per sweep; 131072 + 1 starts the second.
  * k_lincomb, k_emit_flat: min(ceil(n / 256), 2048) workgroups, one element per thread -> 2048 * 256 = 524288 per sweep.
  * k_commit: min(ceil(n / 4 / 256), 2048) workgroups, one float4 per thread -> 2048 * 256 * 4 = 2097152 elements per sweep;
    2097152 + 5 = one float4 of a second sweep + a tail of one (ten buffers of 8.4 MB).
  * 1, 3: tail only; 4: one float4; 5, 255, 1027: float4 + tail.

Tolerances: 8 x the largest deviation of the restatement run in fp32 on the CPU from its fp64 run (helpers.SC_DEV_*, measured and
kept true by the host test) -- the kernels sum in another order.  The ratio recovered from dt_next as (0.9 dt / dt_next)^10 gets
10 x that for the tenth power.  Copies (commit, untouched buffers, sentinels) are compared bit for bit.  Every decision case lies
at least 10 % away from a ratio of 1 (asserted on the reference by the host test): no "one decision apart" is tolerated here."""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL_RATIO = 8 * H.SC_DEV_RATIO          # 4e-6: dt_next (and 10 x: the recovered ratio, 4e-5)
TOL_INIT = 8 * H.SC_DEV_INIT            # 1.28e-6: h0, initial dt
TOL_STAGE = 8 * H.SC_DEV_STAGE          # 4.8e-7 of max|y| per element; stage times, relative
TOL_DENSE = 8 * H.SC_DEV_DENSE          # 3.4e-5 of max|y| per element
SENTINEL = -12345.5
FAR = 10.0

_CASES = {}


def _case(name):
    if name not in _CASES:
        kw = {n: k for n, k, _ in H.SC_STEP_CASES}[name]
        _CASES[name] = H.sc_case(**kw)
    st = _CASES[name]            # (the cached arrays are never written: every user copies)
    return dict(st, y=[a.copy() for a in st['y']], y1=[a.copy() for a in st['y1']], k=[[a.copy() for a in k] for k in st['k']])


def _lib():
    from neural_ode_features_amd import _lib
    return _lib


def _make(st, n_targets=1):
    from neural_ode_features_amd.generic import FlatSolve
    fs = FlatSolve(st['numels'], st['scalar'] is not None, st['rtol'], st['atol'], torch.device('cuda', 0), n_targets)
    _upload(fs, st)
    return fs


def _upload(fs, st):
    for i in range(fs.nseg):
        fs.y[i].copy_(torch.from_numpy(st['y'][i]))
        fs.y1[i].copy_(torch.from_numpy(st['y1'][i]))
        for j in range(7):
            fs.k[i][j].copy_(torch.from_numpy(st['k'][i][j]))
        fs.stage[i].fill_(SENTINEL)


def _dev1(v):
    return torch.tensor([float(v)], dtype=torch.float32, device='cuda')


def _set_scalar(fs, value, ks):
    """The scalar segment through node_flat_scalar: which = -1 (value) and 0..6, accumulate 0 and 1, three scales.  A first write of
    garbage must be overwritten by accumulate = 0; 2 v - v and v / 2 + v / 2 are exact in fp32, fused or not."""
    junk = _dev1(777.0)
    v = _dev1(value)
    fs.scalar(-1, junk, 1.0, False)
    fs.scalar(-1, v, 2.0, False)
    fs.scalar(-1, v, -1.0, True)
    for j, kj in enumerate(ks):
        a = _dev1(kj)
        fs.scalar(j, junk, 1.0, False)
        fs.scalar(j, a, 0.5, False)
        fs.scalar(j, a, 0.5, True)


def _snap(fs):
    torch.cuda.synchronize()
    return dict(y=[t.cpu().numpy() for t in fs.y], y1=[t.cpu().numpy() for t in fs.y1],
                k=[[t.cpu().numpy() for t in ks] for ks in fs.k])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _status(fs):
    s = fs.status()
    return dict(done=s.done, status=s.status, steps=s.steps, accepted=s.accepted, rejected=s.rejected, t=s.t, dt=s.dt,
                first_dt=s.first_dt, scalar=s.scalar)


def _assert_close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.max(np.abs(got - want))) if got.size else 0.0
    print('  %-28s max |dev - fp64| = %.3e (bound %.3e)' % (what, err, tol))
    assert got.shape == want.shape and err <= tol, (what, err, tol)


def _begin(fs, st, targets, tsign=1.0, new_solve=True):
    fs.begin(st['t'], targets, tsign, first_dt=st['dt'], new_solve=new_solve)
    if st['scalar'] is not None and new_solve:
        _set_scalar(fs, st['scalar'][0], st['scalar'][1])


def _check_step(fs, st, targets, j, before, got, y_out=None, y_out_before=None, counts=(0, 0), steps_before=0):
    """Everything one finish_step(dopri5) leaves behind against the restatement.  `before` = the buffers before the step."""
    d = H.sc_finish_step(st, targets, j)
    s = _status(fs)
    print('  ratios', [float('%.6g' % float(r)) for r in d['ratios']], 'accept', d['accept'], 'regime', d['regime'], '->', s)
    acc, rej = counts
    assert s['status'] == d['status'] and s['done'] == int(d['done'])
    assert s['accepted'] == acc + int(d['accept']) and s['rejected'] == rej + int(not d['accept']) and s['steps'] == steps_before + 1
    assert s['t'] == d['t']                                     # t + dt in fp64 on both sides: exact
    if steps_before == 0:
        assert s['first_dt'] == st['dt']
    if d['regime'] == 'free':
        assert abs(s['dt'] / d['dt_next'] - 1) <= TOL_RATIO, (s['dt'], d['dt_next'])
        rec = (0.9 * st['dt'] / s['dt']) ** 10                  # the device's largest ratio, from its unclamped dt_next
        print('  recovered ratio %.8g, fp64 %.8g, relative deviation %.3e (bound %.3e)' % (rec, d['maxr'], abs(rec / d['maxr'] - 1), 10 * TOL_RATIO))
        assert abs(rec / d['maxr'] - 1) <= 10 * TOL_RATIO
    else:
        assert s['dt'] == d['dt_next'], (s['dt'], d['dt_next'])  # x 10, / 1 and / 5 are exact in fp64
    # the buffers
    committed = d['accept'] and not d['done']
    ymax = max(float(np.abs(a).max()) for a in before['y'])      # max|y| of the case
    for i in range(fs.nseg):
        for j6 in range(1, 7):
            assert _same_bits(got['k'][i][j6], before['k'][i][j6]), ('k', i, j6)
        assert _same_bits(got['y1'][i], before['y1'][i]), ('y1', i)
        if committed:
            assert _same_bits(got['y'][i], before['y1'][i]) and _same_bits(got['k'][i][0], before['k'][i][6]), ('commit', i)
        else:
            assert _same_bits(got['k'][i][0], before['k'][i][0]), ('k0', i)
            if d['final'] is None:
                assert _same_bits(got['y'][i], before['y'][i]), ('y', i)
            else:
                _assert_close(got['y'][i], d['final'][0][i], TOL_DENSE * ymax, 'final segment %d' % i)
    if st['scalar'] is not None:
        # (one element has no max|y| of a tensor to lean on: the scale is the sum of the magnitudes its formula adds up)
        v0, sk = abs(float(st['scalar'][0])), [abs(float(x)) for x in st['scalar'][1]]
        if d['final'] is not None:
            _assert_close(s['scalar'], d['final'][1], TOL_DENSE * (v0 + abs(float(d['s_new'])) + st['dt'] * sum(sk)), 'final scalar')
        elif d['accept']:
            scale = v0 + st['dt'] * sum(abs(float(c)) * x for c, x in zip(H.SC_CSOL, sk))
            _assert_close(s['scalar'], d['s_new'], TOL_STAGE * scale, 'scalar after the step')
        else:
            assert np.float32(s['scalar']) == np.float32(st['scalar'][0])
    if y_out is not None:
        rows = y_out.cpu().numpy()
        for r in range(rows.shape[0]):
            if r in d['rows']:
                _assert_close(rows[r], d['rows'][r], TOL_DENSE * ymax, 'dense output row %d' % r)
            else:
                assert _same_bits(rows[r], y_out_before[r]), ('row', r)
    return d, s


# ---------------------------------------------------------------------------------------------------------------------
# stage states and stage times
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tsign', [1.0, -1.0])
@pytest.mark.parametrize('numels', [[n] for n in H.SC_SMALL] + [[H.SC_N_ERR], [5, 1027], [H.SC_N_ERR, 7, 1]], ids=str)
def test_stage_states_and_times(numels, tsign):
    L = _lib()
    rng = np.random.default_rng(sum(numels))
    st = dict(numels=numels, scalar=None, rtol=1e-3, atol=1e-4, t=0.25, dt=0.0625,
              y=[np.concatenate([[2.0], rng.standard_normal(n - 1)]).astype(np.float32) for n in numels],      # max|y| >= 2 at every size
              k=[[rng.standard_normal(n).astype(np.float32) for _ in range(7)] for n in numels])
    st['y1'] = [a.copy() for a in st['y']]
    fs = _make(st)
    _begin(fs, st, [FAR], tsign)
    fs.stage_state(L.METHOD_DOPRI5, L.FLAT_F0)
    torch.cuda.synchronize()
    assert float(fs.t_stage[0]) == float(np.float32(tsign) * np.float32(st['t']))
    assert all(bool((s == SENTINEL).all()) for s in fs.stage)                        # FLAT_F0 writes the time only
    for method, name, stages in ((L.METHOD_DOPRI5, 'dopri5', range(6)), (L.METHOD_RK4, 'rk4', (1, 2, 3))):
        for stage in stages:
            for s in fs.stage:
                s.fill_(SENTINEL)
            out = [t.cpu().numpy() for t in fs.stage_state(method, stage)]
            tdev = float(fs.t_stage[0])
            for i in range(len(numels)):
                want, tw = H.sc_stage(st['y'][i], st['k'][i], st['t'], st['dt'], tsign, stage, name)
                _assert_close(out[i], want, TOL_STAGE * float(np.abs(st['y'][i]).max()), '%s stage %d segment %d' % (name, stage, i))
            _assert_close(tdev, tw, TOL_STAGE * abs(float(tw)), '%s stage %d time' % (name, stage))
    got = _snap(fs)
    for i in range(len(numels)):                                                     # the inputs are only read
        assert _same_bits(got['y'][i], st['y'][i]) and all(_same_bits(got['k'][i][j], st['k'][i][j]) for j in range(7))


# ---------------------------------------------------------------------------------------------------------------------
# Hairer's initial step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,tsign', [(n, 1.0) for n in H.SC_INIT_CASES] + [('n1027', -1.0), ('seg3', -1.0)])
def test_initial_step(name, tsign):
    L = _lib()
    c = H.sc_init_case(name)
    sc = c['scalar']
    rtol, atol = H.SC_INIT_TOL
    m = H.sc_initial_step(c['y'], c['f0'], lambda h0: (c['f1'], None if sc is None else sc[2]), rtol, atol, None if sc is None else sc[:2])
    numels = [a.size for a in c['y']]
    zeros = [np.zeros(n, np.float32) for n in numels]
    st = dict(numels=numels, scalar=None if sc is None else (sc[0], [sc[1]] + [0.0] * 6), rtol=rtol, atol=atol, t=0.0, dt=0.0,
              y=c['y'], y1=zeros, k=[[c['f0'][i]] + [zeros[i]] * 6 for i in range(len(numels))])
    fs = _make(st)
    _begin(fs, st, [FAR], tsign)
    fs.initial_step(0)
    probe = [t.cpu().numpy() for t in fs.stage_state(L.METHOD_DOPRI5, L.FLAT_PROBE)]
    t_probe = float(fs.t_stage[0])
    for i in range(len(numels)):
        fs.k[i][1].copy_(torch.from_numpy(c['f1'][i]))
    if sc is not None:
        fs.scalar(1, _dev1(sc[2]), 1.0, False)
    fs.initial_step(1)
    s = _status(fs)
    print('  fp64 h0 %.9g dt %.9g; device probe time %.9g dt %.9g' % (m['h0'], m['dt'], t_probe, s['dt']))
    assert abs(t_probe / (tsign * m['h0']) - 1) <= TOL_INIT                          # t0 = 0: the probe time IS tsign * h0
    for i in range(len(numels)):
        want = H.sc_stage(c['y'][i], [c['f0'][i]], 0.0, 0.0, tsign, H.SC_PROBE, h0=m['h0'])[0]
        tol = TOL_STAGE * float(np.abs(c['y'][i]).max()) + TOL_INIT * m['h0'] * float(np.abs(c['f0'][i]).max())
        _assert_close(probe[i], want, tol, 'probe state segment %d' % i)
    if name == 'f_zero':
        assert s['dt'] == H.SC_TINY_H                                                # max(1e-6, 1e-3 h0) with h0 = 1e-6: no arithmetic
    else:
        assert abs(s['dt'] / m['dt'] - 1) <= TOL_INIT, (s['dt'], m['dt'])
    assert (s['done'], s['status'], s['steps'], s['accepted'], s['rejected'], s['t']) == (0, 0, 0, 0, 0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# error norm, decision, commit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n, _, _ in H.SC_STEP_CASES])
def test_error_norm_decision_and_commit(name):
    L = _lib()
    st = _case(name)
    fs = _make(st)
    _begin(fs, st, [st['t'] + FAR])
    y_out = torch.full((1, st['numels'][0]), SENTINEL, dtype=torch.float32, device='cuda')
    fs.finish_step(L.METHOD_DOPRI5, y_out)
    d, s = _check_step(fs, st, [st['t'] + FAR], 0, st, _snap(fs), y_out, np.full((1, st['numels'][0]), SENTINEL, np.float32))
    band = {n: b for n, _, b in H.SC_STEP_CASES}[name]
    assert d['accept'] == (band in ('free', 'clamp', 'zero'))
    if band == 'clamp':
        assert s['dt'] == st['dt']
    if band == 'huge':
        assert s['dt'] == st['dt'] / 5
    if band == 'zero':
        assert s['dt'] == st['dt'] * 10


def test_stale_partials_of_a_big_solve_do_not_reach_a_small_one_on_the_same_workspace():
    L = _lib()
    big, small = _case('sweep2'), _case('n5')
    fb = _make(big)
    _begin(fb, big, [big['t'] + FAR])
    fb.finish_step(L.METHOD_DOPRI5, None)
    _check_step(fb, big, [big['t'] + FAR], 0, big, _snap(fb))
    fsm = _make(small)
    fsm.s.ws, fsm.s.ws_bytes = fb.s.ws, fb.s.ws_bytes          # the big solve's controller and its 512 partial sums
    _begin(fsm, small, [small['t'] + FAR])
    fsm.finish_step(L.METHOD_DOPRI5, None)
    _check_step(fsm, small, [small['t'] + FAR], 0, small, _snap(fsm))


@pytest.mark.parametrize('where', ['y1', 'k6_tail'])
@pytest.mark.parametrize('bad', [float('nan'), float('inf')], ids=['nan', 'inf'])
def test_non_finite_input_stops_the_solve_and_commits_nothing(bad, where):
    L = _lib()
    st = _case('n1027')
    if where == 'y1':
        st['y1'][0][517] = bad
    else:
        st['k'][0][6][1026] = bad
    fs = _make(st)
    _begin(fs, st, [st['t'] + FAR])
    fs.finish_step(L.METHOD_DOPRI5, None)
    s, got = _status(fs), _snap(fs)
    print(' ', s)
    assert s['status'] == H.SC_NONFINITE and s['done'] == 1 and s['accepted'] == 0 and s['steps'] == 1
    assert s['t'] == st['t'] and s['dt'] == st['dt']
    assert _same_bits(got['y'][0], st['y'][0]) and _same_bits(got['y1'][0], st['y1'][0])
    assert all(_same_bits(got['k'][0][j], st['k'][0][j]) for j in range(7))


# ---------------------------------------------------------------------------------------------------------------------
# dense output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', H.SC_DENSE_SIZES)
def test_dense_output_rows_over_three_steps(n):
    """Step 1 passes three targets (the third exactly t + dt), step 2 one, step 3 none: rows [j0, j1) get the quartic, every other
    row keeps what it held.  Steps 2 and 3 start from the device's own dt (an input here, checked against fp64 the step before)."""
    L = _lib()
    st, targets = H.sc_dense_scenario(n)
    fs = _make(st, len(targets))
    _begin(fs, st, targets)
    y_out = torch.full((len(targets), n), SENTINEL, dtype=torch.float32, device='cuda')
    j, counts, passed = 0, (0, 0), []
    for step in range(3):
        rows_before = y_out.cpu().numpy()
        fs.finish_step(L.METHOD_DOPRI5, y_out)
        d, s = _check_step(fs, st, targets, j, st, _snap(fs), y_out, rows_before, counts, step)
        passed.append((d['j0'], d['j1']))
        j, counts = d['j1'], (s['accepted'], s['rejected'])
        st = H.sc_advance(st, d, s['dt'])
    assert passed == [(0, 3), (3, 4), (4, 4)]
    torch.cuda.synchronize()
    assert bool((y_out[4] == SENTINEL).all())


@pytest.mark.parametrize('aug', [False, True])
def test_a_step_enqueued_after_done_changes_nothing(aug):
    L = _lib()
    st = _case('seg2_scalar' if aug else 'n1027')
    targets = [st['t'] + 0.6 * st['dt']]
    fs = _make(st)
    _begin(fs, st, targets)
    y_out = torch.full((1, st['numels'][0]), SENTINEL, dtype=torch.float32, device='cuda')
    fs.finish_step(L.METHOD_DOPRI5, y_out)
    d, s1 = _check_step(fs, st, targets, 0, st, _snap(fs), y_out, np.full((1, st['numels'][0]), SENTINEL, np.float32))
    assert d['done'] and s1['done'] == 1
    b1, rows1 = _snap(fs), y_out.cpu().numpy()
    fs.finish_step(L.METHOD_DOPRI5, y_out)
    s2, b2 = _status(fs), _snap(fs)
    assert s2 == s1, (s1, s2)
    assert _same_bits(y_out.cpu().numpy(), rows1)
    for i in range(fs.nseg):
        assert _same_bits(b2['y'][i], b1['y'][i]) and _same_bits(b2['y1'][i], b1['y1'][i])
        assert all(_same_bits(b2['k'][i][j], b1['k'][i][j]) for j in range(7))


# ---------------------------------------------------------------------------------------------------------------------
# augmented final commit, RK4 end of step, second interval
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg2_scalar', 'seg3_scalar'])
def test_augmented_final_commit_overwrites_every_segment_with_the_dense_output(name):
    L = _lib()
    st = _case(name)
    targets = [st['t'] + 0.6 * st['dt']]
    fs = _make(st)
    _begin(fs, st, targets)
    y_out = torch.full((1, st['numels'][0]), SENTINEL, dtype=torch.float32, device='cuda')
    fs.finish_step(L.METHOD_DOPRI5, y_out)
    d, s = _check_step(fs, st, targets, 0, st, _snap(fs), y_out, np.full((1, st['numels'][0]), SENTINEL, np.float32))
    assert d['done'] and d['final'] is not None and s['done'] == 1


@pytest.mark.parametrize('name', ['seg2_scalar', 'sweep2'])
def test_rk4_end_of_step(name):
    L = _lib()
    st = _case(name)
    fs = _make(st)
    _begin(fs, st, [st['t'] + st['dt']])
    fs.finish_step(L.METHOD_RK4, None)
    s, got = _status(fs), _snap(fs)
    for i in range(fs.nseg):
        want = H.sc_rk4_finish(st['y'][i], st['k'][i], st['dt'])
        _assert_close(got['y'][i], want, TOL_STAGE * float(np.abs(st['y'][i]).max()), 'rk4 update segment %d' % i)
        assert _same_bits(got['y1'][i], got['y'][i]) and all(_same_bits(got['k'][i][j], st['k'][i][j]) for j in range(7))
    if st['scalar'] is not None:
        v, sk = st['scalar']
        scale = abs(float(v)) + st['dt'] / 8 * (abs(float(sk[0])) + 3 * abs(float(sk[1])) + 3 * abs(float(sk[2])) + abs(float(sk[3])))
        _assert_close(s['scalar'], H.sc_rk4_finish_scalar(v, sk, st['dt']), TOL_STAGE * scale, 'rk4 scalar')


def test_second_interval_keeps_the_counters_and_the_scalar():
    L = _lib()
    st = _case('seg2_scalar')
    far = [st['t'] + FAR]
    fs = _make(st)
    _begin(fs, st, far)
    fs.finish_step(L.METHOD_DOPRI5, None)
    d, s1 = _check_step(fs, st, far, 0, st, _snap(fs))
    assert d['accept'] and (s1['accepted'], s1['rejected']) == (1, 0)
    st2 = H.sc_advance(st, d, st['dt'] / 4)
    st2['scalar'] = (np.float32(s1['scalar']), st2['scalar'][1])        # (the device's own value: an input of the second interval)
    st2['t'] = 2.0
    _begin(fs, st2, [2.0 + FAR], new_solve=False)
    s = _status(fs)
    assert (s['done'], s['status'], s['steps'], s['accepted'], s['rejected'], s['t'], s['dt']) == (0, 0, 0, 1, 0, 2.0, st['dt'] / 4)
    assert np.float32(s['scalar']) == np.float32(s1['scalar'])
    ratios, _, _ = H.sc_error_ratios(st2['y'], st2['y1'], st2['k'], st2['dt'], st2['rtol'], st2['atol'], st2['scalar'])
    assert all(not (0.9 <= float(r) <= 1.1) for r in ratios), ratios         # the reference alone: the decision is not a close call
    fs.finish_step(L.METHOD_DOPRI5, None)
    _check_step(fs, st2, [2.0 + FAR], 0, st2, _snap(fs), counts=(1, 0))

"""GPU: the finetune evaluation (csrc/kernels_svm.hip, finetune.py, `evaluate.py finetune`) against the fp64 optimum of the
reference's objective and against sklearn's GridSearchCV(LinearSVC) (evaluate.py:364-413).

The fixtures (tests/golden/make_golden_finetune.py) hold, per problem, the fp64 minimiser w* of LinearSVC's objective, and
per C the distance `dz_ref` at which the reference's own converged solver (LinearSVC(dual=False), default tol, float32
features) stops from it.  The fp32 solver may be twice as far, plus the rounding of one fp32 dot product:

    |z - z*| <= 2 dz_ref(C) + (D + 1) 2^-24 (|x|.|w*| + |b*|)            on held-out rows.

A held-out sample whose fp64 top-two margin is below 4 dz_ref(C) (twice that distance, on both sides) is a knife-edge
sample and is left out of prediction comparisons; their share is at most 5 % in every (fold, C).

Measured on an MI355X at the default eps (profiles/finetune_parity.txt): |z - z*| reaches at most 0.2 of its bound, and the
objective gap (f(w) - f*) / f* at most 0.1 of the reference's own `gap_ref(C)`; the factor of 10 allowed below is the issue's.
"""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('small', 'tiny', 'pair', 'wide')


@functools.lru_cache(maxsize=None)
def _golden(name):
    z = dict(np.load(os.path.join(GOLDEN, 'finetune_%s.npz' % name)))
    if 'Xq' in z:
        z['X'] = z['Xq'].astype(np.float32) * z['scale']
    n = len(z['labels'])
    z['xt'] = np.concatenate([z['X'].astype(np.float64), np.ones((n, 1))], 1)
    z['c_index'] = np.array([int(np.argmin(np.abs(z['Cs'] - c))) for c in z['prob_C']])
    z['kk'] = z['z_star'].shape[1]
    return z


def _device(z):
    dev = torch.device('cuda')
    return (torch.from_numpy(z['X']).to(dev), torch.from_numpy(z['labels']).to(dev), torch.from_numpy(z['fold_ids']).to(dev))


@functools.lru_cache(maxsize=None)
def _fit(name):
    """One solve of the golden problem table per fixture, shared by the tests (and left unchanged by them)."""
    from neural_ode_features_amd.finetune import linear_svc_fit, problem_table
    z = _golden(name)
    x, y, f = _device(z)
    table = problem_table(z['prob_fold'], z['prob_class'], z['prob_C'])
    w, info = linear_svc_fit(x, y, f, table)
    return table, w, info


def _z_bound(z, p, rows):
    ci, d1 = z['c_index'][p], z['xt'].shape[1]
    return 2.0 * z['dz_ref'][ci] + d1 * 2.0 ** -24 * (np.abs(z['xt'][rows]) @ np.abs(z['w_star'][p]))


@pytest.mark.parametrize('name', FIXTURES)
def test_solver_reaches_the_fp64_optimum(name):
    z = _golden(name)
    _, w, info = _fit(name)
    assert info['converged'].all(), (info['iterations'].max(), info['grad_ratio'].max())
    w = w.cpu().numpy().astype(np.float64)
    worst = 0.0
    for p, fold in enumerate(z['prob_fold']):
        if fold < 0:
            continue
        held = z['fold_ids'] == fold
        err = np.abs(z['xt'][held] @ w[p] - z['xt'][held] @ z['w_star'][p])
        bound = _z_bound(z, p, held)
        worst = max(worst, (err / bound).max())
        assert (err <= bound).all(), (name, p, fold, z['prob_C'][p], err.max(), bound.min())
    print('%s: iterations <= %d, |z - z*| / bound <= %.3f' % (name, info['iterations'].max(), worst))


def _objective_gaps(z, w):
    gaps = np.zeros(len(z['Cs']))
    for p, fold in enumerate(z['prob_fold']):
        train = z['fold_ids'] != fold
        y = np.where(z['labels'] == z['prob_class'][p], 1.0, -1.0)[train]
        h = np.maximum(0.0, 1.0 - y * (z['xt'][train] @ w[p]))
        f = 0.5 * w[p] @ w[p] + z['prob_C'][p] * (h @ h)
        ci = z['c_index'][p]
        gaps[ci] = max(gaps[ci], (f - z['f_star'][p]) / z['f_star'][p])
    return gaps


@pytest.mark.parametrize('name', FIXTURES)
def test_objective_gap_against_the_reference_solvers(name):
    z = _golden(name)
    gaps = _objective_gaps(z, _fit(name)[1].cpu().numpy().astype(np.float64))
    for c, gap, ref in zip(z['Cs'], gaps, z['gap_ref']):
        print('%s C=%g: (f - f*) / f* = %.3e, reference %.3e' % (name, c, gap, ref))
    assert (gaps <= 10.0 * z['gap_ref']).all(), (gaps, z['gap_ref'])


def _optimum_predictions(z):
    """argmax z* per C on every row (each row is held out by exactly one fold), first maximum on ties."""
    if z['kk'] == 1:
        return z['classes'][(z['z_star'][:, 0] > 0).astype(np.int64)]
    return z['classes'][z['z_star'].argmax(1)]


def _held_out_predictions(name):
    from neural_ode_features_amd.finetune import svc_cv_score
    z = _golden(name)
    table, w, _ = _fit(name)
    x, y, f = _device(z)
    n_groups = 5 * len(z['Cs'])
    groups = np.arange(n_groups * z['kk']).reshape(n_groups, z['kk'])          # the table is ordered (fold, C, class)
    correct, held, pred = svc_cv_score(x, y, f, table, w, groups, neg_class=int(z['classes'][0]), return_pred=True)
    return correct.reshape(5, -1), held.reshape(5, -1), pred.reshape(5, len(z['Cs']), -1)


@pytest.mark.parametrize('name', FIXTURES)
def test_held_out_predictions_equal_the_optimums_outside_the_knife_edge(name):
    z = _golden(name)
    correct, held, pred = _held_out_predictions(name)
    want = _optimum_predictions(z)
    for fold in range(5):
        rows = z['fold_ids'] == fold
        assert (held[fold] == rows.sum()).all()
        for ci in range(len(z['Cs'])):
            knife = z['knife'][ci][rows]
            assert knife.mean() <= 0.05, (name, fold, ci, knife.mean())
            got = pred[fold, ci]
            assert (got[~rows] == -1).all()
            assert (got[rows][~knife] == want[ci][rows][~knife]).all(), (name, fold, ci)
            assert correct[fold, ci] == (got[rows] == z['labels'][rows]).sum()
            acc_star = (want[ci][rows] == z['labels'][rows]).mean()
            assert abs(correct[fold, ci] / rows.sum() - acc_star) <= knife.sum() / rows.sum() + 1e-12, (name, fold, ci)


@pytest.mark.parametrize('name', ['small', 'tiny'])
def test_grid_search_matches_sklearn(name):
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import LinearSVC
    from neural_ode_features_amd.finetune import linear_svc_cv
    z = _golden(name)
    x, y, _ = _device(z)
    search = linear_svc_cv(x, y, Cs=z['Cs'])
    assert search.converged.all()
    assert np.array_equal(search.row_fold, z['fold_ids']) and np.array_equal(search.classes, z['classes'])
    correct, held, _ = _held_out_predictions(name)
    assert np.array_equal(search.fold_correct, correct) and np.array_equal(search.fold_sizes, held)
    assert np.array_equal(search.fold_scores, correct / held)
    assert np.array_equal(search.mean_test_score, (correct / held).mean(0))
    assert search.best_index == int(np.argmax(search.mean_test_score))           # numpy's argmax: the first maximum
    assert search.best_C == z['Cs'][search.best_index] and search.best_score == search.mean_test_score[search.best_index]
    # per C the scores can differ from sklearn's only on knife-edge samples; so the maxima differ by at most the largest
    sizes = np.bincount(z['fold_ids'])
    allowance = max(sum(z['knife'][ci][z['fold_ids'] == f].sum() / sizes[f] for f in range(5)) / 5 for ci in range(len(z['Cs'])))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        live = GridSearchCV(LinearSVC(dual=False), {'C': z['Cs']}, scoring='accuracy', cv=5).fit(z['X'], z['labels'])
    assert abs(search.best_score - live.best_score_) <= allowance + 1e-12, (search.best_score, live.best_score_, allowance)
    assert abs(search.best_score - float(z['best_score'])) <= allowance + 1e-12, (search.best_score, z['best_score'], allowance)
    # the refit at the best C against the golden refit optimum: the bound of the optimum test, on every row
    kk = z['kk']
    refit = np.flatnonzero((z['prob_fold'] == -1) & (z['c_index'] == search.best_index))
    assert len(refit) == kk and search.coef.shape == (kk, z['X'].shape[1]) and search.intercept.shape == (kk,)
    rows = np.ones(len(z['labels']), bool)
    for ki, p in enumerate(refit):
        w = np.concatenate([search.coef[ki], search.intercept[ki:ki + 1]]).astype(np.float64)
        err = np.abs(z['xt'] @ w - z['xt'] @ z['w_star'][p])
        assert (err <= _z_bound(z, p, rows)).all(), (name, p, err.max())


def test_runs_are_bit_identical_and_independent_of_the_column_order():
    from neural_ode_features_amd.finetune import linear_svc_fit
    z = _golden('small')
    x, y, f = _device(z)
    table, w1, info1 = _fit('small')
    w2, info2 = linear_svc_fit(x, y, f, table)
    assert torch.equal(w1, w2) and np.array_equal(info1, info2)
    perm = np.random.default_rng(0).permutation(len(table))
    w3, info3 = linear_svc_fit(x, y, f, table[perm])
    assert torch.equal(w3, w1[torch.from_numpy(perm).to(w1.device)]) and np.array_equal(info3, info1[perm])


def test_max_iter_zero_returns_zeros_and_not_converged():
    from neural_ode_features_amd.finetune import linear_svc_fit
    z = _golden('tiny')
    x, y, f = _device(z)
    w, info = linear_svc_fit(x, y, f, _fit('tiny')[0], max_iter=0)
    assert float(w.abs().max()) == 0.0
    assert not info['converged'].any() and (info['iterations'] == 0).all()
    # one iteration is not enough either, and says so
    w, info = linear_svc_fit(x, y, f, _fit('tiny')[0], max_iter=1)
    assert not info['converged'].all() and (info['iterations'] <= 1).all() and float(w.abs().max()) > 0.0


def test_finetune_mode_end_to_end(tmp_path):
    """train -> features -> finetune on a run directory; every cv_accuracy against a live sklearn grid search on the same
    slice, within the slice's own knife-edge allowance (make_golden_finetune.reference_solution on that slice)."""
    import pandas as pd
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    from neural_ode_features_amd.finetune import predict
    sys.path.insert(0, GOLDEN)
    try:
        from make_golden_finetune import ALL_CS, reference_solution
    finally:
        sys.path.remove(GOLDEN)
    run = str(tmp_path / 'run')
    assert T.main(['--dataset', 'mnist', '-f', '16', '-b', '32', '--synthetic-size', '1200', '-a', '--lr', '0.05', '-e', '2',
                   '--run-dir', run]) == 0
    E.main(['features', run, '--t1', '0', '0.5', '1', '--tol', '1e-3', '--limit', '200'])
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)          # a problem that did not converge would warn
        df = pd.read_csv(E.main(['finetune', run]))
    assert list(df.columns) == ['block', 't1', 'cv_accuracy', 'tol']
    assert df.block.tolist() == [0, 0, 0] and df.t1.tolist() == [0.0, 0.5, 1.0] and df.tol.tolist() == [1e-3] * 3
    f = np.load(os.path.join(run, 'features.npz'))
    feats, y_true = f['features'][0], f['y_true']
    assert feats.shape == (3, 200, 16)
    for i, t1 in enumerate((0.0, 0.5, 1.0)):
        ref, _ = reference_solution(feats[i], y_true, ALL_CS)
        sizes = np.bincount(ref['fold_ids'])
        allowance = max(sum(ref['knife'][ci][ref['fold_ids'] == k].sum() / sizes[k] for k in range(5)) / 5 for ci in range(5))
        print('t1 %g: cv_accuracy %.4f, sklearn %.4f, allowance %.4f' % (t1, df.cv_accuracy[i], ref['best_score'], allowance))
        assert abs(df.cv_accuracy[i] - ref['best_score']) <= allowance + 1e-12, (t1, df.cv_accuracy[i], ref['best_score'], allowance)
        svm = np.load(os.path.join(run, 'svms', 'svm_b0_t%g.npz' % t1))
        ci = int(np.argmin(np.abs(ALL_CS - float(svm['C']))))
        assert svm['coef'].shape == (10, 16) and svm['intercept'].shape == (10,) and np.array_equal(svm['classes'], np.arange(10))
        # the stored refit predicts what the refit optimum at that C predicts, outside ITS knife-edge rows
        star = ref['w_star'][(ref['prob_fold'] == -1) & (np.abs(ref['prob_C'] - ALL_CS[ci]) < 1e-12 * ALL_CS[ci])]
        zs = np.concatenate([feats[i].astype(np.float64), np.ones((200, 1))], 1) @ star.T
        top = np.sort(zs, axis=1)
        safe = top[:, -1] - top[:, -2] >= 4.0 * ref['dz_ref'][ci]
        got = predict(svm['coef'], svm['intercept'], svm['classes'], feats[i])
        assert (got[safe] == zs.argmax(1)[safe]).all()
    df = pd.read_csv(E.main(['finetune', run, '--aggregate']))
    assert df.block.tolist() == [0] and df.t1.tolist() == [-1] and df.tol.tolist() == [1e-3]
    assert os.path.exists(os.path.join(run, 'svms', 'svm_b0_t-1.npz'))

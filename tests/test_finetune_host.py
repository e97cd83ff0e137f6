"""CPU-side checks of the finetune evaluation (finetune.py, csrc/svm_api.hip, `evaluate.py finetune`): the fold assignment
against sklearn and the golden fixtures, the refusals of the C ABI, and the mode's bookkeeping with the solver stubbed out.
No compute: there is no GPU here."""
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('small', 'tiny', 'pair', 'wide')


@pytest.mark.parametrize('name', FIXTURES)
def test_stratified_folds_equal_the_golden_fold_ids(name):
    from neural_ode_features_amd.finetune import stratified_folds
    z = np.load(os.path.join(GOLDEN, 'finetune_%s.npz' % name))
    folds = stratified_folds(z['labels'])
    assert folds.dtype == np.int32
    assert np.array_equal(folds, z['fold_ids'])


def test_stratified_folds_equal_sklearn_on_unequal_unsorted_classes():
    from sklearn.model_selection import StratifiedKFold
    from neural_ode_features_amd.finetune import stratified_folds
    rng = np.random.default_rng(0)
    # classes 7, 2, 9, 4 appear in that order, with 23, 5, 11 and 38 members
    y = np.concatenate([[7, 2, 9, 4], rng.permutation(np.repeat([7, 2, 9, 4], [22, 4, 10, 37]))])
    for k in (5, 3, 2):
        want = np.empty(len(y), np.int32)
        for f, (_, test) in enumerate(StratifiedKFold(k).split(np.zeros((len(y), 1)), y)):
            want[test] = f
        assert np.array_equal(stratified_folds(y, k), want), k
    with pytest.raises(ValueError, match='fewer than the 5 folds'):
        stratified_folds(np.array([0] * 10 + [1] * 4))


def test_workspace_bytes_grow_and_refusals_need_no_device():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    base = lib.node_svm_workspace_bytes(603, 33, 300)
    assert base > 0 and base % 256 == 0
    assert lib.node_svm_workspace_bytes(1206, 33, 300) > base
    assert lib.node_svm_workspace_bytes(603, 66, 300) > base
    assert lib.node_svm_workspace_bytes(603, 33, 600) > base
    assert lib.node_svm_workspace_bytes(1, 1, 1) > 0
    # the problems run in chunks above 256 MiB: the Tiny-ImageNet grid (K = 200, P = 6000) stays near the bound
    assert lib.node_svm_workspace_bytes(10000, 256, 6000) <= (256 << 20) + (16 << 20)
    for args, word in (((0, 33, 300), 'n=0'), ((603, 0, 300), 'd=0'), ((603, 33, 0), 'p=0'), ((603, 281, 300), 'at most 280')):
        assert lib.node_svm_workspace_bytes(*args) == 0, args
        assert word in lib.node_last_error().decode(), (args, lib.node_last_error())
    dummy = 256      # never dereferenced: every refusal below happens on the host
    fit = lambda n=603, d=33, p=300, x=dummy, prob=dummy, eps=1e-5, it=10, ws=dummy, nb=1 << 30: lib.node_svm_fit(
        n, d, p, x, dummy, dummy, prob, eps, it, dummy, dummy, ws, nb, None)
    assert fit(n=0) == -2 and 'n=0' in lib.node_last_error().decode()                            # NODE_ERR_SHAPE
    assert fit(d=281) == -3 and 'at most 280' in lib.node_last_error().decode()                  # NODE_ERR_UNSUPPORTED
    assert fit(x=None) == -1 and 'NULL' in lib.node_last_error().decode()                        # NODE_ERR_NULL
    assert fit(prob=None) == -1 and 'NULL' in lib.node_last_error().decode()
    assert fit(ws=None) == -1 and 'NULL' in lib.node_last_error().decode()
    assert fit(eps=0.0) == -9 and 'eps' in lib.node_last_error().decode()                        # NODE_ERR_ARG
    assert fit(it=-1) == -9 and 'max_iter=-1' in lib.node_last_error().decode()
    assert fit(nb=16) == -4 and 'workspace too small' in lib.node_last_error().decode()          # NODE_ERR_WORKSPACE
    score = lambda n=603, g=25, k=10, w=dummy: lib.node_svm_cv_score(n, 33, 300, g, k, dummy, dummy, dummy, dummy, w, dummy, 0,
                                                                     dummy, dummy, None, None)
    assert score(n=0) == -2 and 'n=0' in lib.node_last_error().decode()
    assert score(g=0) == -2 and 'n_groups=0' in lib.node_last_error().decode()
    assert score(k=0) == -2 and 'k=0' in lib.node_last_error().decode()
    assert score(w=None) == -1 and 'NULL' in lib.node_last_error().decode()


def test_python_wrappers_refuse_bad_arguments():
    from neural_ode_features_amd import finetune as F
    x = torch.rand(40, 6)
    y = torch.arange(40) % 4
    with pytest.raises(RuntimeError, match='no CPU path'):
        F.linear_svc_cv(x, y)
    with pytest.raises(RuntimeError, match='no CPU path'):
        F.linear_svc_fit(x, y, np.zeros(40, np.int32), ([0], [1], [1.0]))
    with pytest.raises(TypeError, match='float32'):
        F.linear_svc_cv(x.double(), y)
    with pytest.raises(ValueError, match='contiguous'):
        F.linear_svc_cv(x.T.contiguous().T, y)
    with pytest.raises(ValueError, match='at most 280'):
        F.linear_svc_cv(torch.rand(40, 281), y)
    with pytest.raises(ValueError, match='eps'):
        F.linear_svc_cv(x, y, eps=0.0)
    with pytest.raises(ValueError, match='max_iter'):
        F.linear_svc_cv(x, y, max_iter=-1)
    with pytest.raises(ValueError, match='finite and > 0'):
        F.problem_table([0], [1], [0.0])
    t = F.problem_table([0, -1], [3, 3], [0.5, 2.0])
    assert t.dtype.itemsize == 12 and t['fold'].tolist() == [0, -1] and t['c'].tolist() == [0.5, 2.0]


def _run_dir(tmp_path, downsample, tols, t1s, n=12, d=3):
    run = tmp_path / 'run'
    run.mkdir()
    torch.save({'params': {'downsample': downsample}, 'model': {}}, run / 'last.pth')
    slices = len(t1s) * (2 if downsample == 'ode' else 1)
    feats = np.arange(len(tols) * slices * n * d, dtype=np.float32).reshape(len(tols), slices, n, d)
    np.savez(run / 'features.npz', features=feats, y_true=np.arange(n) % 3, tols=np.array(tols), t1s=np.array(t1s))
    return str(run), feats


def test_finetune_mode_refuses_a_run_without_features(tmp_path):
    from neural_ode_features_amd import evaluate as E
    run = tmp_path / 'empty'
    run.mkdir()
    with pytest.raises(SystemExit, match='run the `features` mode first'):
        E.main(['finetune', str(run)])


@pytest.mark.parametrize('downsample', ['residual', 'ode'])
def test_finetune_mode_bookkeeping_with_the_solver_stubbed(tmp_path, monkeypatch, downsample):
    import pandas as pd
    from neural_ode_features_amd import evaluate as E
    tols, t1s = [1e-3, 1e-1], [0.0, 0.5, 1.0]
    run, feats = _run_dir(tmp_path, downsample, tols, t1s)
    seen = []

    def stub(fi, y_true):
        seen.append(np.array(fi))
        return types.SimpleNamespace(best_score=float(fi.mean()), best_C=1.0, coef=np.zeros((3, fi.shape[1])),
                                     intercept=np.zeros(3), classes=np.unique(y_true))

    monkeypatch.setattr(E, '_svc_search', stub)
    df = pd.read_csv(E.main(['finetune', run]))
    assert list(df.columns) == ['block', 't1', 'cv_accuracy', 'tol']
    blocks = [0, 0, 0, 1, 1, 1] if downsample == 'ode' else [0, 0, 0]
    ts = t1s * 2 if downsample == 'ode' else t1s
    assert df.block.tolist() == blocks * 2 and df.t1.tolist() == ts * 2
    assert df.tol.tolist() == [tols[0]] * len(ts) + [tols[1]] * len(ts)
    want = feats.reshape(-1, *feats.shape[2:])
    assert len(seen) == len(want) and all(np.array_equal(a, b) for a, b in zip(seen, want))
    assert np.allclose(df.cv_accuracy.to_numpy(), want.mean((1, 2)))
    for b, t in zip(blocks, ts):
        for tol in tols:
            f = np.load(os.path.join(run, 'svms', 'svm_b%d_t%g_tol%g.npz' % (b, t, tol)))
            assert f['coef'].shape == (3, 3) and f['intercept'].shape == (3,) and float(f['C']) == 1.0

    # --aggregate: the mean over the T axis of each tolerance slice, t1 = -1, one row per tolerance (zip keeps the reference's
    # single slice for an `ode` stem too)
    del seen[:]
    df = pd.read_csv(E.main(['finetune', run, '--aggregate']))
    assert df.block.tolist() == [0, 0] and df.t1.tolist() == [-1, -1] and df.tol.tolist() == tols
    assert len(seen) == 2 and all(np.allclose(a, feats[i].mean(0)) for i, a in enumerate(seen))
    assert os.path.exists(os.path.join(run, 'svms', 'svm_b0_t-1_tol0.001.npz'))


def test_finetune_mode_names_the_svm_file_without_tol_for_one_tolerance(tmp_path, monkeypatch):
    from neural_ode_features_amd import evaluate as E
    run, _ = _run_dir(tmp_path, 'residual', [0], [0.0, 1.0])
    monkeypatch.setattr(E, '_svc_search', lambda fi, y: types.SimpleNamespace(
        best_score=0.5, best_C=0.1, coef=np.zeros((3, 3)), intercept=np.zeros(3), classes=np.arange(3)))
    E.main(['finetune', run, '-a'])
    assert sorted(os.listdir(os.path.join(run, 'svms'))) == ['svm_b0_t-1.npz']

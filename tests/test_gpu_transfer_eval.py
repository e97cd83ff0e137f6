"""GPU: the transfer evaluations (`evaluate.py features / retrieval / finetune -d NAME`, the reference's evaluate.py:30, 38-51,
311-312, 368-371) end to end on a run directory: a net trained on 32-pixel images extracts the features of a file of
64-pixel images.

The features are compared with those of the same model fed the images that the numpy restatement of
tests/test_resize_host.py resizes and numpy normalises, in the same batches.  The inputs are bit-identical, so the bound,
1e-6 absolute, allows for nothing more than the run-to-run identity of the solve on 8 x 8 states."""
import os

import numpy as np
import pytest
import torch

from tests.test_resize_host import resize

pytestmark = pytest.mark.gpu

NAME = 'tiny-imagenet-200'
CIFAR10 = ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))


def test_transfer_features_retrieval_and_finetune(tmp_path):
    import pandas as pd
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    run = str(tmp_path / 'run')
    assert T.main(['--dataset', 'cifar10', '-f', '16', '-b', '32', '--synthetic-size', '64', '-a', '-e', '1', '--run-dir', run]) == 0
    rng = np.random.default_rng(17)
    x = rng.integers(0, 256, (60, 3, 64, 64), dtype=np.uint8)
    y = np.arange(60, dtype=np.int64) % 3
    x += (y * 40).astype(np.uint8)[:, None, None, None]               # (wraps: the classes differ, that is all)
    blob = str(tmp_path / 'tiny_val.pt')
    torch.save({'x_test': torch.from_numpy(x), 'y_test': torch.from_numpy(y)}, blob)

    out = E.main(['features', run, '-d', NAME, '--data-file', blob, '--t1', '0', '0.5', '1', '--tol', '1e-3'])
    assert out == os.path.join(run, 'features-%s.npz' % NAME) and os.path.exists(out)
    assert not os.path.exists(os.path.join(run, 'features.npz'))
    z = np.load(out)
    assert z['features'].shape == (1, 3, 60, 16) and np.array_equal(z['y_true'], y)
    assert z['t1s'].tolist() == [0.0, 0.5, 1.0] and z['tols'].tolist() == [1e-3]

    # the same model on the restatement's inputs, in the same batches
    mean, std = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in CIFAR10)
    inputs = (resize(x, 32, 32).astype(np.float32) / np.float32(255) - mean) / std
    assert inputs.dtype == np.float32 and inputs.shape == (60, 3, 32, 32)
    model, p, _, _ = E.load_run(run)
    assert p.batch_size == 32 and p.augmentation == 'none'            # normalised all the same: evaluate.py:49
    model = model.cuda().eval()
    model.to_features_extractor()
    model.odeblock.t1, model.odeblock.tol = [0.0, 0.5, 1.0], 1e-3
    with torch.no_grad():
        want = np.concatenate([model(torch.from_numpy(inputs[i:i + 32]).cuda()).cpu().numpy() for i in range(0, 60, 32)], -2)
    err = float(np.abs(z['features'][0] - want).max())
    print('features of the transfer set: max |difference| %.3e (bound 1e-6), max |feature| %.3e' % (err, np.abs(want).max()))
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-3
    assert err <= 1e-6

    df = pd.read_csv(E.main(['retrieval', run, '-d', NAME]))
    assert os.path.exists(os.path.join(run, 'retrieval-%s.csv' % NAME)) and not os.path.exists(os.path.join(run, 'retrieval.csv'))
    assert list(df.columns) == ['ap_asym', 'ap_sym', 'ap10_asym', 'ap10_sym', 't1', 'tol'] and len(df) == 3 * 60
    df = pd.read_csv(E.main(['finetune', run, '-d', NAME]))
    assert os.path.exists(os.path.join(run, 'finetune-%s.csv' % NAME)) and not os.path.exists(os.path.join(run, 'finetune.csv'))
    assert list(df.columns) == ['block', 't1', 'cv_accuracy', 'tol'] and df.t1.tolist() == [0.0, 0.5, 1.0]
    assert ((df.cv_accuracy >= 0) & (df.cv_accuracy <= 1)).all()
    svms = os.path.join(run, 'svms-%s' % NAME)
    assert sorted(os.listdir(svms)) == ['svm_b0_t0.5.npz', 'svm_b0_t0.npz', 'svm_b0_t1.npz'] and not os.path.exists(os.path.join(run, 'svms'))
    assert np.load(os.path.join(svms, 'svm_b0_t1.npz'))['coef'].shape == (3, 16)
    # without the switch the modes go on reading the run's own files
    with pytest.raises(SystemExit, match='features.npz'):
        E.main(['finetune', run])


def test_a_channel_mismatch_exits_with_a_message(tmp_path):
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import evaluate as E
    run = tmp_path / 'run'
    run.mkdir()
    params = dict(dataset='mnist', data=None, seed=23, synthetic_size=64, batch_size=32, filters=16, downsample='residual',
                  method='dopri5', tol=1e-3, adjoint=True, dropout=0, norm='group', augmentation='none')
    torch.save({'epoch': 1, 'params': params, 'model': nof.ODENet(1, out=10, n_filters=16, adjoint=True).state_dict()}, str(run / 'last.pth'))
    blob = str(tmp_path / 'colour.pt')
    torch.save({'x_test': torch.zeros(6, 3, 64, 64, dtype=torch.uint8), 'y_test': torch.zeros(6, dtype=torch.int64)}, blob)
    with pytest.raises(SystemExit, match='3-channel images.*1-channel'):
        E.main(['features', str(run), '-d', NAME, '--data-file', blob])
    assert not os.path.exists(str(run / ('features-%s.npz' % NAME)))

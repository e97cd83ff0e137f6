"""GPU: the input pipeline (csrc/kernels_augment.hip through augment.Augmenter) against the independent fp64 restatement of
tests/test_augment_host.py, and training through `--augmentation`.

Tolerance: 1e-5 in PIXEL units ([0, 1] scale), i.e. 1e-5 / std[c] on a normalised output.  Basis: the same formulas in numpy
fp32 against fp64 differ by at most 1.1e-6 over 4 M random pixels, near-grey ones included (measured on the CPU); the composite
map is continuous, also across hue sectors and ties of the channel maximum; the bound leaves about 9 x for FMA contraction and
the device's division.  Any misplaced pixel, wrong offset, wrong fill or wrong flip direction is an error of >= 1 / 255."""
import csv
import os

import numpy as np
import pytest
import torch

from tests.test_augment_host import CIFAR10, KIND_FLAGS, restate

pytestmark = pytest.mark.gpu

N = 37
TOL = 1e-5
SEED, EPOCH = 23, 3
MNIST_STATS = ((0.1307,), (0.3081,))
SHAPES = {'mnist': ((1, 28, 28), 4), 'cifar': ((3, 32, 32), 4), 'odd': ((3, 12, 20), 3)}      # (C, H, W), padding


def _coded(shape):
    """Pixels that encode (item, channel, row, column); never 0, so the zero fill cannot be mistaken for data."""
    c, h, w = shape
    item, ch, row, col = np.meshgrid(np.arange(N), np.arange(c), np.arange(h), np.arange(w), indexing='ij')
    return (1 + (item * 89 + ch * 53 + row * 31 + col * 7) % 255).astype(np.uint8)


def _random(shape, seed):
    """Random 8-bit images; for colour, items 0..3 are near-grey (channels within +-1 of each other) and item 4 starts with
    rows of pure primaries, secondaries, black and white."""
    c, h, w = shape
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (N, c, h, w), dtype=np.uint8)
    if c == 3:
        base = rng.integers(1, 255, (4, 1, h, w))
        data[:4] = np.clip(base + rng.integers(-1, 2, (4, 3, h, w)), 0, 255).astype(np.uint8)
        colours = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)]
        for r, rgb in enumerate(colours):
            data[4, :, r] = np.asarray(rgb, dtype=np.uint8)[:, None]
    return data


def _indices(batch, seed):
    rng = np.random.default_rng(seed)
    index = rng.integers(0, N, batch)
    index[:min(batch, 5)] = np.arange(5)[:batch]             # the near-grey items and the primaries are in every batch > 4
    if batch >= 7:
        index[5:7] = 4, 4                                    # repeats, also in the small batch
    return index.astype(np.int64)


@pytest.fixture(scope='module')
def labels():
    return np.random.default_rng(7).integers(0, 10, N).astype(np.int64)


def _augmenter(kind, name, seed=SEED):
    import neural_ode_features_amd as nof
    shape, padding = SHAPES[name]
    mean, std = (MNIST_STATS if shape[0] == 1 else CIFAR10) if KIND_FLAGS[kind] & 8 else (None, None)
    return nof.Augmenter(kind, mean=mean, std=std, padding=padding, seed=seed), mean, std


def _run(kind, name, data, labels, index, epoch=EPOCH, seed=SEED, train=True):
    import neural_ode_features_amd as nof
    aug, mean, std = _augmenter(kind, name, seed)
    split = nof.DeviceSplit(torch.from_numpy(data), torch.from_numpy(labels), 'cuda')
    images, target = aug.batch(split, torch.from_numpy(index).cuda(), epoch, train=train)
    assert images.dtype == torch.float32 and images.shape == (len(index),) + data.shape[1:] and target.dtype == torch.int64
    return images.cpu().numpy(), target.cpu().numpy(), mean, std


def _pixel_error(got, want, std):
    err = np.abs(got.astype(np.float64) - want)
    if std is not None:
        err = err * np.asarray(std)[None, :, None, None]
    return float(err.max())


@pytest.mark.parametrize('batch', [1, 7, 130])
@pytest.mark.parametrize('name', ['mnist', 'cifar', 'odd'])
def test_crop_geometry_and_label_gather(name, batch, labels):
    shape, padding = SHAPES[name]
    data, index = _coded(shape), _indices(batch, 100 + batch)
    got, target, _, _ = _run('crop', name, data, labels, index)
    want, want_labels = restate(data, labels, index, EPOCH, SEED, KIND_FLAGS['crop'], padding)
    err = _pixel_error(got, want, None)
    print('crop %s batch %d: max error %.3e (bound %.0e)' % (name, batch, err, TOL))
    assert np.array_equal(target, want_labels)
    assert err <= TOL
    assert (got == 0).any() or batch == 1                     # some image of the batch was shifted: zero fill is in play


@pytest.mark.parametrize('batch', [1, 7, 130])
@pytest.mark.parametrize('kind,name', [('crop+flip+norm', 'mnist'), ('crop+flip+norm', 'cifar'), ('crop+flip+norm', 'odd'),
                                       ('crop+jitter+flip+norm', 'cifar'), ('crop+jitter+flip+norm', 'odd')])
def test_full_chain_against_the_fp64_restatement(kind, name, batch, labels):
    shape, padding = SHAPES[name]
    data, index = _random(shape, 11), _indices(batch, 200 + batch)
    got, target, mean, std = _run(kind, name, data, labels, index)
    want, want_labels = restate(data, labels, index, EPOCH, SEED, KIND_FLAGS[kind], padding, 0.05, 0.05, mean, std)
    err = _pixel_error(got, want, std)
    print('%s %s batch %d: max error %.3e pixel units (bound %.0e)' % (kind, name, batch, err, TOL))
    assert np.array_equal(target, want_labels)
    assert err <= TOL


def test_an_image_does_not_depend_on_its_batch(labels):
    data = _random(SHAPES['cifar'][0], 12)
    kind = 'crop+jitter+flip+norm'
    big = _indices(130, 5)
    big[77] = 5
    one = _run(kind, 'cifar', data, labels, np.array([5], dtype=np.int64))[0][0]
    three = _run(kind, 'cifar', data, labels, np.array([5, 9, 5], dtype=np.int64))[0]
    many = _run(kind, 'cifar', data, labels, big)[0]
    assert np.array_equal(one, three[0]) and np.array_equal(one, three[2]) and np.array_equal(one, many[77])
    assert not np.array_equal(one, three[1])
    assert not np.array_equal(one, _run(kind, 'cifar', data, labels, np.array([5], dtype=np.int64), epoch=EPOCH + 1)[0][0])
    assert not np.array_equal(one, _run(kind, 'cifar', data, labels, np.array([5], dtype=np.int64), seed=SEED + 1)[0][0])
    assert not np.array_equal(one, _run(kind, 'cifar', data, labels, np.array([5], dtype=np.int64), seed=SEED + (1 << 32))[0][0])


@pytest.mark.parametrize('kind,name', [('crop', 'mnist'), ('none', 'odd'), ('crop+flip+norm', 'odd'), ('crop+jitter+flip+norm', 'cifar')])
def test_the_test_transform_consumes_no_draw(kind, name, labels):
    shape, _ = SHAPES[name]
    data, index = _random(shape, 13), _indices(130, 6)
    got, target, mean, std = _run(kind, name, data, labels, index, train=False)
    want = data[index].astype(np.float64) / 255.0
    if std is not None:
        want = (want - np.asarray(mean)[None, :, None, None]) / np.asarray(std)[None, :, None, None]
    err = _pixel_error(got, want, std)
    print('test transform %s %s: max error %.3e pixel units (bound %.0e)' % (kind, name, err, TOL))
    assert err <= TOL and np.array_equal(target, labels[index])
    other = _run(kind, name, data, labels, index, epoch=EPOCH + 5, seed=SEED + 9, train=False)[0]
    assert np.array_equal(got, other)
    if kind == 'none':                                        # 'none' is the test transform in training, too
        assert np.array_equal(got, _run(kind, name, data, labels, index, train=True)[0])


def test_an_index_outside_the_split_reads_nothing(labels):
    data = _random(SHAPES['odd'][0], 14)
    index = np.array([3, N, -1, 1 << 40, 36], dtype=np.int64)
    import neural_ode_features_amd as nof
    split = nof.DeviceSplit(torch.from_numpy(data), torch.from_numpy(labels), 'cuda')
    images, target = nof.Augmenter('none').batch(split, torch.from_numpy(index).cuda(), 0)
    assert target.tolist() == [int(labels[3]), -1, -1, -1, int(labels[36])]
    assert float(images[1:4].abs().max()) == 0.0
    assert np.array_equal(images[4].cpu().numpy(), (data[36].astype(np.float32) / np.float32(255)))
    with pytest.raises(RuntimeError, match='no CPU path'):
        nof.Augmenter('none').batch(split, torch.from_numpy(index), 0)


def test_train_with_the_augmentation_flag_in_both_loops_and_evaluate(tmp_path):
    """`--augmentation crop+jitter+flip+norm` through the read-back loop and through `--deferred`: what
    tests/test_gpu_train.py asserts of the two loops, on batches that come from Augmenter.batch; the checkpoint records the
    flag, and `evaluate features` runs on the run with the test transform."""
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    common = ['--dataset', 'cifar10', '--augmentation', 'crop+jitter+flip+norm', '-f', '64', '-b', '32', '--synthetic-size', '96',
              '-a', '-e', '2']
    sync, blind = str(tmp_path / 'sync'), str(tmp_path / 'blind')
    assert T.main(common + ['--run-dir', sync]) == 0
    assert T.main(common + ['--run-dir', blind, '--deferred']) == 0
    a = list(csv.DictReader(open(os.path.join(sync, 'log.csv'))))
    b = list(csv.DictReader(open(os.path.join(blind, 'log.csv'))))
    assert [int(r['epoch']) for r in a] == [int(r['epoch']) for r in b] == [1, 2]
    for k in ('loss', 'acc', 'nfe-f', 'nfe-b', 'test_loss', 'test_acc', 'test_nfe'):
        assert k in a[0] and k in b[0]
    assert float(a[0]['nfe-f']) >= 14 and float(a[0]['nfe-b']) >= 15
    for ra, rb in zip(a, b):
        assert np.isfinite(float(ra['loss'])) and np.isfinite(float(rb['loss']))
        assert abs(float(ra['loss']) - float(rb['loss'])) < 2e-2 * max(1.0, abs(float(ra['loss'])))
        assert abs(float(ra['nfe-f']) - float(rb['nfe-f'])) <= 6.0 and abs(float(ra['nfe-b']) - float(rb['nfe-b'])) <= 6.0
        assert abs(float(ra['test_acc']) - float(rb['test_acc'])) <= 0.1
    ck = torch.load(os.path.join(sync, 'last.pth'), map_location='cpu', weights_only=False)
    assert set(ck) == {'epoch', 'params', 'model', 'optim', 'metrics'} and ck['epoch'] == 2
    assert ck['params']['augmentation'] == 'crop+jitter+flip+norm'
    out = E.main(['features', sync, '--t1', '0', '1', '--tol', '1e-3', '--limit', '24'])
    z = np.load(out)
    assert z['features'].shape == (1, 2, 24, 64) and z['y_true'].shape == (24,) and np.isfinite(z['features']).all()
    model, p, xte, yte = E.load_run(sync)
    assert xte.is_cuda and xte.dtype == torch.float32 and p.augmentation == 'crop+jitter+flip+norm'
    raw = T.load_data(p)[2]
    mean, std = torch.tensor(CIFAR10[0]).view(1, 3, 1, 1), torch.tensor(CIFAR10[1]).view(1, 3, 1, 1)
    assert float(((xte.cpu() - (raw.float() / 255 - mean) / std).abs() * std).max()) <= TOL

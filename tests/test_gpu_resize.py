"""GPU: the transfer transform (csrc/kernels_resize.hip through augment.TransferTransform) against Pillow's outputs
(tests/golden/resize_pil.npz) and the independent numpy restatement of tests/test_resize_host.py.

The resample is integer arithmetic on bytes, and the fp32 output uses the expressions of the input pipeline's test transform
on the same bytes: a misplaced tap, a transposed pass order or a float intermediate is an error of at least one grey level
somewhere in these cases.  Exact equality is therefore the bound everywhere; no tolerance is measured."""
import functools

import numpy as np
import pytest
import torch

from tests.test_resize_host import golden, resize

pytestmark = pytest.mark.gpu

N = 37
CIFAR10 = ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
TINY = ((0.4802, 0.4481, 0.3975), (0.2770, 0.2691, 0.2821))
# (C, H, W, OH, OW): the golden size pairs, plus widths that are no multiple of 4 on either side and one tap per output (2 -> 1)
SHAPES = [c for c, _, _ in golden()] + [(3, 7, 13, 11, 6), (1, 64, 64, 1, 1), (3, 6, 2, 3, 1)]


@functools.lru_cache(maxsize=None)
def _data(c, h, w):
    rng = np.random.default_rng(c * 10007 + h * 101 + w)
    data = rng.integers(0, 256, (N, c, h, w), dtype=np.uint8)
    data[1] = 255
    data[2] = rng.integers(0, 2, (c, h, w), dtype=np.uint8) * 255
    data.setflags(write=False)
    labels = rng.integers(0, 10, N).astype(np.int64)
    labels.setflags(write=False)
    return data, labels


@functools.lru_cache(maxsize=None)
def _want(c, h, w, oh, ow):
    """The restatement on all N items, computed once per shape and shared."""
    out = resize(_data(c, h, w)[0], oh, ow)
    out.setflags(write=False)
    return out


def _split(data, labels):
    import neural_ode_features_amd as nof
    return nof.DeviceSplit(torch.from_numpy(np.array(data)), torch.from_numpy(np.array(labels)), 'cuda')


@pytest.mark.parametrize('k', range(8))
def test_resized_equals_pillow_bit_for_bit(k):
    import neural_ode_features_amd as nof
    (c, h, w, oh, ow), x, want = golden()[k]
    split = _split(x, np.arange(3, dtype=np.int64))
    got = nof.TransferTransform((oh, ow)).resized(split, torch.arange(3, device='cuda'))
    assert got.dtype == torch.uint8 and got.shape == (3, c, oh, ow)
    got = got.cpu().numpy()
    print('%s: %d of %d bytes differ' % ((c, h, w, oh, ow), int((got != want).sum()), want.size))
    assert np.array_equal(got, want)
    assert (got[1] == 255).all()                              # all 255 stays 255: the rounding constant and the coefficient sums


@pytest.mark.parametrize('batch', [1, 7])
@pytest.mark.parametrize('shape', SHAPES)
def test_resized_equals_the_restatement_and_labels_follow_the_index(shape, batch):
    import neural_ode_features_amd as nof
    c, h, w, oh, ow = shape
    data, labels = _data(c, h, w)
    index = np.array([36, 1, 5, 5, 2, 0, 36], dtype=np.int64)[:batch]            # repeated, out of order
    got, target = nof.TransferTransform((oh, ow))._launch(_split(data, labels), torch.from_numpy(index).cuda(), False)
    assert np.array_equal(target.cpu().numpy(), labels[index])
    assert np.array_equal(got.cpu().numpy(), _want(*shape)[index]), shape


def test_every_item_and_both_outputs_of_one_launch_agree():
    """All 37 items in one batch at the reference's two pairings; `.batch` is ToTensor + Normalize of `.resized`'s bytes."""
    import neural_ode_features_amd as nof
    for shape, (mean, std) in (((3, 32, 32, 64, 64), TINY), ((3, 64, 64, 32, 32), CIFAR10)):
        c, h, w, oh, ow = shape
        data, labels = _data(c, h, w)
        split = _split(data, labels)
        order = torch.arange(N, device='cuda')
        tt = nof.TransferTransform(oh, mean=mean, std=std)
        pixels = tt.resized(split, order)
        assert np.array_equal(pixels.cpu().numpy(), _want(*shape))
        images, target = tt.batch(split, order)
        assert images.dtype == torch.float32 and images.shape == (N, c, oh, ow) and np.array_equal(target.cpu().numpy(), labels)
        aug = nof.Augmenter('crop+flip+norm', mean=mean, std=std)
        want, _ = aug.batch(nof.DeviceSplit(pixels, split.y, 'cuda'), order, 0, train=False)
        assert torch.equal(images, want)
        again, _ = tt.batch(split, order)
        assert torch.equal(images, again) and torch.equal(pixels, tt.resized(split, order))          # two launches: bit-equal


@pytest.mark.parametrize('shape', [(1, 28, 28, 64, 64), (3, 20, 36, 9, 50), (3, 7, 13, 11, 6)])
def test_batch_equals_the_test_transform_of_the_resized_bytes(shape):
    import neural_ode_features_amd as nof
    c, h, w, oh, ow = shape
    data, labels = _data(c, h, w)
    split = _split(data, labels)
    index = torch.tensor([3, 36, 3, 0, 1, 2, 20], device='cuda')
    mean, std = (((0.1307,), (0.3081,)) if c == 1 else CIFAR10)
    resized = nof.DeviceSplit(nof.TransferTransform((oh, ow)).resized(split, index), split.y[index], 'cuda')
    order = torch.arange(len(index), device='cuda')
    for stats in ((mean, std), (None, None)):
        images, _ = nof.TransferTransform((oh, ow), mean=stats[0], std=stats[1]).batch(split, index)
        aug = nof.Augmenter('crop+flip+norm', mean=mean, std=std) if stats[0] else nof.Augmenter('none')
        assert torch.equal(images, aug.batch(resized, order, 0, train=False)[0]), (shape, stats)


def test_the_identity_size_is_the_plain_test_transform():
    import neural_ode_features_amd as nof
    for c, h, w in ((3, 32, 32), (3, 7, 13)):
        data, labels = _data(c, h, w)
        split = _split(data, labels)
        index = torch.tensor([5, 1, 36, 5], device='cuda')
        tt = nof.TransferTransform((h, w), dataset='cifar10')
        assert torch.equal(tt.resized(split, index), split.x[index])
        images, target = tt.batch(split, index)
        want, want_target = nof.Augmenter('crop+flip+norm', dataset='cifar10').batch(split, index, 0, train=False)
        assert torch.equal(images, want) and torch.equal(target, want_target)


def test_an_index_outside_the_split_reads_nothing():
    import neural_ode_features_amd as nof
    data, labels = _data(3, 32, 32)
    split = _split(data, labels)
    index = torch.tensor([3, N, -1, 1 << 40, 36], device='cuda')
    tt = nof.TransferTransform(64, dataset='tiny-imagenet-200')
    pixels, target = tt._launch(split, index, False)
    assert target.tolist() == [int(labels[3]), -1, -1, -1, int(labels[36])]
    assert int(pixels[1:4].max()) == 0 and np.array_equal(pixels[4].cpu().numpy(), _want(3, 32, 32, 64, 64)[36])
    images, _ = tt.batch(split, index)
    black = (-torch.tensor(TINY[0]) / torch.tensor(TINY[1])).cuda().view(1, 3, 1, 1)
    assert float((images[1:4] - black).abs().max()) <= 1e-6 and torch.equal(images[1], images[2]) and torch.equal(images[1], images[3])
    assert bool((images[1] == images[1][:, :1, :1]).all())               # one value per channel
    assert tt.batch(split, index[:0])[0].shape == (0, 3, 64, 64)


def test_sizes_out_of_range_are_refused():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd._lib import NodeHipError
    data = np.random.default_rng(4).integers(0, 256, (2, 1, 257, 8), dtype=np.uint8)
    split = _split(data, np.zeros(2, dtype=np.int64))
    index = torch.arange(2, device='cuda')
    with pytest.raises(NotImplementedError, match='on chip') as info:          # 257 * 256 bytes between the passes
        nof.TransferTransform((4, 256)).resized(split, index)
    assert isinstance(info.value, NodeHipError) and info.value.code == -3
    got = nof.TransferTransform((4, 255)).resized(split, index)                                   # 65535 bytes: served
    assert np.array_equal(got.cpu().numpy(), resize(data, 4, 255))
    with pytest.raises(RuntimeError, match='no CPU path'):
        nof.TransferTransform(4).resized(split, index.cpu())


def test_the_largest_intermediate_is_served():
    """h * out_w = 65536 bytes exactly, the whole of the limit (the tables then stay in global memory): against the restatement."""
    import neural_ode_features_amd as nof
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, (2, 1, 256, 8), dtype=np.uint8)
    got = nof.TransferTransform((3, 256)).resized(_split(data, np.zeros(2, dtype=np.int64)), torch.arange(2, device='cuda'))
    assert np.array_equal(got.cpu().numpy(), resize(data, 3, 256))

"""CPU-side checks of the input pipeline (csrc/kernels_augment.hip, csrc/augment_api.hip, augment.py) and the independent
restatement the GPU tests compare the kernel with (tests/test_gpu_augment.py imports it from here).

The restatement is numpy only and shares no code with the package: Philox4x32-10 on uint64 arithmetic, the draws as
include/node_hip.h words them, and the pixel math of torchvision's tensor backend (adjust_saturation, adjust_hue) in fp64.
It is itself checked against the Random123 known-answer vectors of Philox4x32-10."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

CROP, JITTER, FLIP, NORM = 1, 2, 4, 8
KIND_FLAGS = {'none': 0, 'crop': CROP, 'crop+flip+norm': CROP | FLIP | NORM, 'crop+jitter+flip+norm': CROP | JITTER | FLIP | NORM}
# utils.py:13-19 of the reference
CIFAR10 = ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
CIFAR100 = ((0.5071, 0.4865, 0.4409), (0.2673, 0.2564, 0.2762))
TINY = ((0.4802, 0.4481, 0.3975), (0.2770, 0.2691, 0.2821))

MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars), key: two -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k = [np.uint64(key[0]) & MASK, np.uint64(key[1]) & MASK]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(0x9E3779B9)) & MASK, (k[1] + np.uint64(0xBB67AE85)) & MASK]
    return [v.astype(np.uint32) for v in c]


def draws(index, epoch, seed, padding, s, h):
    """The per-image random numbers: dy, dx in {0 .. 2 padding}, flip, hue_first (bool), fs, fh (float32)."""
    index = np.asarray(index, dtype=np.int64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = philox4x32_10((index, epoch, 0, 0), key)
    span = np.uint64(2 * padding + 1)
    dy = ((w[0].astype(np.uint64) * span) >> np.uint64(32)).astype(np.int64)
    dx = ((w[1].astype(np.uint64) * span) >> np.uint64(32)).astype(np.int64)
    flip, hue_first = (w[2] >> np.uint32(31)).astype(bool), (w[3] >> np.uint32(31)).astype(bool)
    v = philox4x32_10((index, epoch, 1, 0), key)

    def unit(x):
        return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    s32, h32 = np.float32(s), np.float32(h)
    fs = (np.float32(1) - s32) + np.float32(2) * s32 * unit(v[0])
    fh = -h32 + np.float32(2) * h32 * unit(v[1])
    assert fs.dtype == np.float32 and fh.dtype == np.float32
    return dy, dx, flip, hue_first, fs, fh


def adjust_saturation(x, fs, dtype=np.float64):
    """x: [3, ...] on [0, 1]."""
    x = x.astype(dtype)
    fs = dtype(fs)
    gray = dtype(0.2989) * x[0] + dtype(0.587) * x[1] + dtype(0.114) * x[2]
    return np.clip(fs * x + (dtype(1) - fs) * gray, 0, 1)


def adjust_hue(x, fh, dtype=np.float64):
    x = x.astype(dtype)
    fh = dtype(fh)
    r, g, b = x
    one = dtype(1)
    maxc, minc = x.max(0), x.min(0)
    eq = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eq, one, maxc)
    crd = np.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (dtype(2) + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (dtype(4) + gc - rc)
    hh = np.fmod((hr + hg + hb) / dtype(6) + one, one)
    hh = np.mod(hh + fh, one)
    v = maxc
    i = np.floor(hh * dtype(6))
    f = hh * dtype(6) - i
    i = i.astype(np.int64) % 6
    p = np.clip(v * (one - s), 0, 1)
    q = np.clip(v * (one - s * f), 0, 1)
    t = np.clip(v * (one - s * (one - f)), 0, 1)
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.zeros_like(x)
    for sector, rgb in enumerate(table):
        for ch in range(3):
            out[ch] = np.where(i == sector, rgb[ch], out[ch])
    return out


def restate(data, labels, index, epoch, seed, flags, padding=0, s=0.05, h=0.05, mean=None, std=None):
    """The transform chain in its own order -- Pad, Crop, Jitter, Flip, ToTensor, Normalize -- in fp64.
    data uint8 [N, C, H, W] -> (float64 [B, C, H, W], int64 [B])."""
    data, labels, index = np.asarray(data), np.asarray(labels), np.asarray(index)
    _, c, hh, ww = data.shape
    dy, dx, flip, hue_first, fs, fh = draws(index, epoch, seed, padding, s, h)
    out = np.zeros((len(index), c, hh, ww))
    for b, item in enumerate(index):
        img = data[item].astype(np.float64) / 255.0
        if flags & CROP:
            padded = np.pad(img, ((0, 0), (padding, padding), (padding, padding)))
            img = padded[:, dy[b]:dy[b] + hh, dx[b]:dx[b] + ww]
        if flags & JITTER:
            if hue_first[b]:
                img = adjust_saturation(adjust_hue(img, fh[b]), fs[b])
            else:
                img = adjust_hue(adjust_saturation(img, fs[b]), fh[b])
        if flags & FLIP and flip[b]:
            img = img[:, :, ::-1]
        if flags & NORM:
            img = (img - np.asarray(mean, dtype=np.float64)[:, None, None]) / np.asarray(std, dtype=np.float64)[:, None, None]
        out[b] = img
    return out, labels[index].astype(np.int64)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    cases = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for counter, key, want in cases:
        got = tuple(int(v) for v in philox4x32_10(counter, key))
        assert got == want, (['%08x' % v for v in got], ['%08x' % v for v in want])
    # vectorised over the first counter word: the same numbers as one call each
    many = philox4x32_10((np.arange(5), 7, 1, 0), (23, 0))
    for i in range(5):
        assert tuple(int(v[i]) for v in many) == tuple(int(v) for v in philox4x32_10((i, 7, 1, 0), (23, 0)))


def test_draw_statistics():
    """8192 dataset indices at a fixed seed and epoch, padding 4: every offset occurs, the coin flips lie within 4 sigma
    (0.5 +- 4 * 0.5 / sqrt(8192) = 0.5 +- 0.022), the jitter factors lie in their half-open intervals."""
    dy, dx, flip, hue_first, fs, fh = draws(np.arange(8192), 3, 23, 4, 0.05, 0.05)
    assert set(dy.tolist()) == set(range(9)) and set(dx.tolist()) == set(range(9))
    assert abs(flip.mean() - 0.5) <= 0.022, flip.mean()
    assert abs(hue_first.mean() - 0.5) <= 0.022, hue_first.mean()
    assert fs.min() >= np.float32(0.95) and fs.max() < np.float32(1.05)
    assert fh.min() >= np.float32(-0.05) and fh.max() < np.float32(0.05)
    # the draws are a function of (seed, epoch, index) alone
    again = draws(np.arange(8192)[::-1], 3, 23, 4, 0.05, 0.05)
    assert np.array_equal(again[0][::-1], dy) and np.array_equal(again[4][::-1], fs)
    other = draws(np.arange(8192), 4, 23, 4, 0.05, 0.05)
    assert not np.array_equal(other[0], dy) and not np.array_equal(other[4], fs)


def test_pixel_math_properties_of_the_restatement():
    """Black stays black (so the zero padding needs no jitter), identity factors are the identity, fp32 follows fp64."""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (3, 4096)).astype(np.float64) / 255.0
    x[:, :64] = x[:1, :64]                                   # greys
    x[:, 64:67] = np.eye(3)                                  # primaries
    x[:, 67] = 0.0
    assert np.array_equal(adjust_hue(np.zeros((3, 5)), 0.03), np.zeros((3, 5)))
    assert np.array_equal(adjust_saturation(np.zeros((3, 5)), 1.04), np.zeros((3, 5)))
    assert np.abs(adjust_hue(x, 0.0) - x).max() < 1e-12
    assert np.abs(adjust_saturation(x, 1.0) - x).max() < 1e-12
    assert np.abs(adjust_hue(x[:, :64], 0.04) - x[:, :64]).max() < 1e-12       # a grey has no hue
    for fs, fh in ((0.95, -0.05), (1.0499, 0.0499), (1.01, 0.02)):
        a = adjust_hue(adjust_saturation(x, fs), fh)
        b = adjust_hue(adjust_saturation(x, fs, np.float32), fh, np.float32)
        assert np.abs(a - b).max() < 5e-6


def test_abi_refusals_without_a_device():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    dummy = 256       # never dereferenced: every refusal below happens on the host

    def desc(n=37, c=3, h=32, w=32, padding=4, flags=CROP | JITTER | FLIP | NORM, s=0.05, hue=0.05, mean=CIFAR10[0], std=CIFAR10[1]):
        d = _lib.NodeAugment(n, c, h, w, padding, flags, s, hue)
        d.mean[:], d.std[:] = mean, std
        return d

    def call(d, data=dummy, labels=dummy, index=dummy, batch=8, out=dummy, out_labels=dummy):
        rc = lib.node_augment_batch(d, data, labels, index, batch, 23, 1, out, out_labels, None)
        return rc, lib.node_last_error().decode()

    assert call(None)[0] == -1
    for kw in ({'data': None}, {'labels': None}, {'index': None}, {'out': None}, {'out_labels': None}):
        rc, msg = call(desc(), **kw)
        assert rc == -1 and 'NULL' in msg, (kw, rc, msg)                              # NODE_ERR_NULL
    for d, kw, word in ((desc(n=0), {}, 'n=0'), (desc(h=0), {}, 'h=0'), (desc(w=-3), {}, 'w=-3'), (desc(), {'batch': 0}, 'batch=0')):
        rc, msg = call(d, **kw)
        assert rc == -2 and word in msg, (rc, msg)                                    # NODE_ERR_SHAPE
    for c in (0, 2, 4):
        rc, msg = call(desc(c=c, flags=CROP))
        assert rc == -3 and 'c=%d' % c in msg, (rc, msg)                              # NODE_ERR_UNSUPPORTED
    rc, msg = call(desc(c=1, mean=(0.5, 0, 0), std=(0.5, 1, 1)))
    assert rc == -3 and 'jitter' in msg and 'c=1' in msg, (rc, msg)
    rc, msg = call(desc(padding=32768))                                               # 2 P + 1 = 65537 > 2^16
    assert rc == -9 and 'padding=32768' in msg, (rc, msg)                             # NODE_ERR_ARG
    rc, msg = call(desc(padding=-1))
    assert rc == -9 and 'padding=-1' in msg, (rc, msg)
    for std in ((0.2, 0.0, 0.2), (0.2, 0.2, -1.0), (float('nan'), 0.2, 0.2)):
        rc, msg = call(desc(std=std))
        assert rc == -9 and 'std' in msg, (std, rc, msg)
    rc, msg = call(desc(flags=16))
    assert rc == -9 and 'flags' in msg, (rc, msg)
    rc, msg = call(desc(s=1.5))
    assert rc == -9 and 'saturation' in msg, (rc, msg)
    rc, msg = call(desc(hue=0.6))
    assert rc == -9 and 'hue' in msg, (rc, msg)


def test_descriptor_layout_matches_the_header(tmp_path):
    import os
    import subprocess
    from neural_ode_features_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ['n', 'c', 'h', 'w', 'padding', 'flags', 'saturation', 'hue', 'mean', 'std']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(node_augment));']
    lines += ['  printf("%s %%zu\\n", offsetof(node_augment, %s));' % (f, f) for f in fields]
    lines += ['  printf("bits %d %d %d %d\\n", NODE_AUG_CROP, NODE_AUG_JITTER, NODE_AUG_FLIP, NODE_AUG_NORM);', '  return 0;', '}']
    src = tmp_path / 'aug.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'aug'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['size']) == C.sizeof(_lib.NodeAugment)
    for f in fields:
        assert int(got[f]) == getattr(_lib.NodeAugment, f).offset, f
    assert [int(v) for v in got['bits'].split()] == [_lib.AUG_CROP, _lib.AUG_JITTER, _lib.AUG_FLIP, _lib.AUG_NORM] == [CROP, JITTER, FLIP, NORM]


def test_augmenter_tables_match_the_reference_settings():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import augment as A
    assert A.KINDS == ('none', 'crop', 'crop+flip+norm', 'crop+jitter+flip+norm') and A.FLAGS == KIND_FLAGS
    assert A.PREPROC['cifar10'] == CIFAR10 and A.PREPROC['cifar100'] == CIFAR100 and A.PREPROC['tiny-imagenet-200'] == TINY
    assert A.PREPROC['mnist'] == ((0.0,), (1.0,))
    assert A.PADDING == {28: 4, 32: 4, 64: 8} and A.SATURATION == A.HUE == 0.05
    assert nof.Augmenter is A.Augmenter and nof.DeviceSplit is A.DeviceSplit
    aug = nof.Augmenter('crop+jitter+flip+norm', dataset='cifar10', seed=23)
    d = aug.descriptor((50000, 3, 32, 32))
    assert (d.n, d.c, d.h, d.w, d.padding, d.flags) == (50000, 3, 32, 32, 4, CROP | JITTER | FLIP | NORM)
    assert abs(d.saturation - 0.05) < 1e-8 and abs(d.hue - 0.05) < 1e-8
    assert np.allclose(list(d.mean), CIFAR10[0], atol=1e-7) and np.allclose(list(d.std), CIFAR10[1], atol=1e-7)
    t = aug.descriptor((10000, 3, 32, 32), train=False)          # the test transform: ToTensor + Normalize
    assert t.flags == NORM and t.padding == 0
    assert nof.Augmenter('crop+flip+norm', dataset='tiny-imagenet-200').descriptor((10, 3, 64, 64)).padding == 8
    m = nof.Augmenter('crop').descriptor((10, 1, 28, 28))
    assert (m.padding, m.flags) == (4, CROP) and nof.Augmenter('crop').descriptor((10, 1, 28, 28), train=False).flags == 0
    assert nof.Augmenter('none').descriptor((10, 1, 28, 28)).flags == 0
    assert nof.Augmenter('crop', padding=3).descriptor((10, 3, 12, 20)).padding == 3
    with pytest.raises(ValueError, match='padding'):
        nof.Augmenter('crop').descriptor((10, 3, 12, 20))        # no reference padding for that size
    with pytest.raises(ValueError, match='one of'):
        nof.Augmenter('flip')
    with pytest.raises(ValueError, match='known dataset'):
        nof.Augmenter('crop+flip+norm')
    with pytest.raises(ValueError, match='3 channels'):
        nof.Augmenter('crop+jitter+flip+norm', mean=(0.5,), std=(0.5,)).descriptor((10, 1, 28, 28))
    with pytest.raises(ValueError, match='std > 0'):
        nof.Augmenter('crop+flip+norm', mean=(0.5, 0.5, 0.5), std=(0.5, 0.0, 0.5))


def test_cpu_tensors_are_refused():
    import neural_ode_features_amd as nof
    x, y = torch.zeros(4, 3, 32, 32, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        nof.DeviceSplit(x, y, 'cpu')
    with pytest.raises(TypeError, match='uint8'):
        nof.DeviceSplit(x.float(), y, 'cuda')
    with pytest.raises(ValueError, match='labels'):
        nof.DeviceSplit(x, y[:3], 'cuda')
    with pytest.raises(TypeError, match='DeviceSplit'):
        nof.Augmenter('crop').batch((x, y), torch.zeros(2, dtype=torch.int64), 0)


def test_train_data_for_the_flag_and_runs_without_it(tmp_path):
    """`--augmentation` wants 8-bit pixels: the synthetic set gets a uint8 form with the same labels, float `--data` exits with
    a message; a checkpoint written before the flag existed has no such key and evaluates as 'none'."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    assert T.AUGMENTATIONS == ('none', 'crop', 'crop+flip+norm', 'crop+jitter+flip+norm')
    base = dict(dataset='cifar10', data=None, seed=23, synthetic_size=64, batch_size=32)
    plain = T.load_data(types.SimpleNamespace(augmentation='none', **base))
    old = T.load_data(types.SimpleNamespace(**base))                 # the params of a run of before the flag
    aug = T.load_data(types.SimpleNamespace(augmentation='crop+jitter+flip+norm', **base))
    assert plain[0].dtype == torch.float32 and torch.equal(plain[0], old[0])
    assert aug[0].dtype == aug[2].dtype == torch.uint8 and aug[0].shape == plain[0].shape == (64, 3, 32, 32)
    assert torch.equal(aug[1], plain[1]) and torch.equal(aug[3], plain[3]) and aug[4:] == plain[4:] == (3, 10)
    assert 16 < aug[0].float().std() < 128                            # not clipped away
    blob = str(tmp_path / 'float.pt')
    torch.save({'x_train': plain[0], 'y_train': plain[1], 'x_test': plain[2], 'y_test': plain[3]}, blob)
    with pytest.raises(SystemExit, match='uint8'):
        T.load_data(types.SimpleNamespace(augmentation='crop', **dict(base, data=blob)))
    assert T.load_data(types.SimpleNamespace(augmentation='none', **dict(base, data=blob)))[0].dtype == torch.float32
    net = nof.ODENet(3, out=10, n_filters=16, adjoint=True)
    params = dict(base, filters=16, downsample='residual', method='dopri5', tol=1e-3, adjoint=True, dropout=0, norm='group')
    run = tmp_path / 'run'
    run.mkdir()
    torch.save({'epoch': 1, 'params': params, 'model': net.state_dict()}, str(run / 'last.pth'))
    model, p, xte, yte = E.load_run(str(run))
    assert xte.dtype == torch.float32 and torch.equal(xte, plain[2]) and not hasattr(p, 'augmentation')

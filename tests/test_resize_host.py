"""CPU-side checks of the transfer transform (csrc/kernels_resize.hip, csrc/resize_api.hip, augment.TransferTransform, the
`-d/--data` switch of evaluate.py) and the independent restatement the GPU tests compare the kernel with
(tests/test_gpu_resize.py and tests/test_gpu_transfer_eval.py import it from here).

The restatement is numpy only and shares no code with the package: PIL's 8-bit bilinear resample as include/node_hip.h words
it -- per axis the double-precision weights, their 22-bit fixed-point coefficients, the horizontal pass rounded to bytes,
then the vertical pass.  It is itself checked against Pillow's outputs (tests/golden/resize_pil.npz, written by
tests/golden/make_golden_resize.py), and against a live Pillow where there is one.  All of it is integer arithmetic, so every
comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resize_pil.npz')
BITS = 22
AXES = [(32, 64), (64, 32), (28, 64), (20, 9), (36, 50), (64, 7), (5, 64), (64, 48)]


def axis_table(n_in, n_out):
    """(xmin [out], count [out], coeff: a list of int64 arrays) of one axis."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = filterscale
    xmins, counts, coeffs = [], [], []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        x = np.arange(xmin, xmax, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((x - center + 0.5) / filterscale))
        total = 0.0
        for v in w:                                   # summed left to right, as a C loop does
            total += v
        w = w / total
        xmins.append(xmin)
        counts.append(xmax - xmin)
        coeffs.append(np.array([int(v * float(1 << BITS) + 0.5) for v in w], dtype=np.int64))
    return np.array(xmins), np.array(counts), coeffs


def resample_last_axis(x, n_out):
    """x uint8 [..., n_in] -> uint8 [..., n_out]; the same size: the pass is skipped."""
    n_in = x.shape[-1]
    if n_in == n_out:
        return x
    xmin, count, coeff = axis_table(n_in, n_out)
    out = np.empty(x.shape[:-1] + (n_out,), dtype=np.uint8)
    for xx in range(n_out):
        acc = (1 << (BITS - 1)) + (x[..., xmin[xx]:xmin[xx] + count[xx]].astype(np.int64) * coeff[xx]).sum(-1)
        assert acc.max() < 2 ** 31
        out[..., xx] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(x, oh, ow):
    """x uint8 [..., H, W] -> uint8 [..., OH, OW]: horizontally first, to bytes, then vertically."""
    x = resample_last_axis(np.asarray(x), ow)
    return np.ascontiguousarray(np.swapaxes(resample_last_axis(np.swapaxes(x, -1, -2), oh), -1, -2))


def golden():
    z = np.load(GOLDEN)
    return [(tuple(int(v) for v in case), z['in_%d' % k], z['out_%d' % k]) for k, case in enumerate(z['cases'])]


def test_the_restatement_equals_the_golden_outputs_of_pillow():
    cases = golden()
    assert [c for c, _, _ in cases] == [(3, 32, 32, 64, 64), (3, 64, 64, 32, 32), (1, 28, 28, 64, 64), (3, 32, 32, 32, 32),
                                        (3, 20, 36, 9, 50), (3, 64, 64, 7, 7), (3, 5, 5, 64, 64), (3, 64, 64, 48, 40)]
    for (c, h, w, oh, ow), x, want in cases:
        assert x.shape == (3, c, h, w) and want.shape == (3, c, oh, ow) and x.dtype == want.dtype == np.uint8
        assert (x[1] == 255).all() and set(np.unique(x[2])) == {0, 255} and len(np.unique(x[0])) > 16
        assert np.array_equal(resize(x, oh, ow), want), (c, h, w, oh, ow)
    assert np.array_equal(cases[3][1], cases[3][2])                   # 32 -> 32 is the identity


def test_the_restatement_equals_a_live_pillow_on_fresh_images():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(5)
    for (c, h, w, oh, ow), _, _ in golden():
        x = rng.integers(0, 256, (2, c, h, w), dtype=np.uint8)
        x[1] = rng.integers(0, 2, (c, h, w), dtype=np.uint8) * 255    # 0 / 255 noise
        want = np.stack([np.asarray(Image.fromarray(p, 'L').resize((ow, oh), Image.BILINEAR)) for p in x.reshape(-1, h, w)])
        assert np.array_equal(resize(x, oh, ow), want.reshape(2, c, oh, ow)), (c, h, w, oh, ow)


def _library_table(n_in, n_out):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    need = lib.node_resize_table(n_in, n_out, None, None, None, 0)
    assert need > 0 and need % n_out == 0, (need, lib.node_last_error())
    xmin, count, coeff = (C.c_int32 * n_out)(), (C.c_int32 * n_out)(), (C.c_int32 * need)()
    assert lib.node_resize_table(n_in, n_out, xmin, count, coeff, need) == need
    return np.array(xmin), np.array(count), np.array(coeff).reshape(n_out, need // n_out)


@pytest.mark.parametrize('n_in,n_out', AXES)
def test_the_library_table_equals_the_restatement(n_in, n_out):
    xmin, count, coeff = _library_table(n_in, n_out)
    want_xmin, want_count, want_coeff = axis_table(n_in, n_out)
    assert np.array_equal(xmin, want_xmin) and np.array_equal(count, want_count)
    assert coeff.shape[1] == 2 * int(np.ceil(max(n_in / n_out, 1.0))) + 1 and count.max() <= coeff.shape[1]
    assert xmin.min() >= 0 and (xmin + count).max() <= n_in and count.min() >= 1          # every tap lies inside the axis
    for xx in range(n_out):
        assert np.array_equal(coeff[xx, :count[xx]], want_coeff[xx]), (n_in, n_out, xx)
        assert not coeff[xx, count[xx]:].any()
        assert abs(int(coeff[xx].sum()) - (1 << BITS)) <= count[xx], (n_in, n_out, xx, coeff[xx].sum())
        assert coeff[xx].min() >= 0


def test_table_capacity_and_refusals():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    need = lib.node_resize_table(64, 7, None, None, None, 0)
    assert need == 7 * (2 * 10 + 1)                                   # support = ceil(64 / 7) = 10
    xmin, count, coeff = (C.c_int32 * 7)(*([-5] * 7)), (C.c_int32 * 7)(), (C.c_int32 * need)()
    assert lib.node_resize_table(64, 7, xmin, count, coeff, need - 1) == need
    assert list(xmin) == [-5] * 7                                     # an undersized capacity writes nothing
    assert lib.node_resize_table(64, 7, xmin, count, coeff, need) == need and list(xmin) != [-5] * 7
    assert lib.node_resize_table(32, 32, None, None, None, 0) == 32 * 3
    assert lib.node_resize_table(64, 7, None, count, coeff, need) == -1 and 'NULL' in lib.node_last_error().decode()
    for n_in, n_out in ((0, 4), (4, 0), (-1, 4)):
        assert lib.node_resize_table(n_in, n_out, None, None, None, 0) == -2          # NODE_ERR_SHAPE
    assert lib.node_resize_table(1 << 30, 1, None, None, None, 0) == -3 and 'coefficients' in lib.node_last_error().decode()


def test_abi_refusals_without_a_device():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    dummy = 256       # never dereferenced: every refusal below happens on the host

    def desc(n=37, c=3, h=32, w=32, out_h=64, out_w=64, normalize=1, mean=(0.5, 0.5, 0.5), std=(0.2, 0.2, 0.2)):
        d = _lib.NodeResize(n, c, h, w, out_h, out_w, normalize)
        d.mean[:], d.std[:] = mean, std
        return d

    def call(d, data=dummy, labels=dummy, index=dummy, batch=8, out_f32=dummy, out_u8=dummy, out_labels=dummy):
        rc = lib.node_resize_batch(d, data, labels, index, batch, out_f32, out_u8, out_labels, None)
        return rc, lib.node_last_error().decode()

    assert call(None)[0] == -1
    for kw in ({'data': None}, {'labels': None}, {'index': None}, {'out_labels': None}, {'out_f32': None, 'out_u8': None}):
        rc, msg = call(desc(), **kw)
        assert rc == -1 and 'NULL' in msg, (kw, rc, msg)                              # NODE_ERR_NULL
    for d, kw, word in ((desc(n=0), {}, 'n=0'), (desc(h=0), {}, 'h=0'), (desc(w=-3), {}, 'w=-3'), (desc(out_h=0), {}, 'out_h=0'),
                        (desc(out_w=0), {}, 'out_w=0'), (desc(), {'batch': 0}, 'batch=0')):
        rc, msg = call(d, **kw)
        assert rc == -2 and word in msg, (rc, msg)                                    # NODE_ERR_SHAPE
    for c in (0, 2, 4):
        rc, msg = call(desc(c=c))
        assert rc == -3 and 'c=%d' % c in msg, (rc, msg)                              # NODE_ERR_UNSUPPORTED
    rc, msg = call(desc(h=257, out_w=256))                                            # 65792 bytes between the passes
    assert rc == -3 and 'h=257' in msg and 'out_w=256' in msg, (rc, msg)
    rc, msg = call(desc(n=1 << 20, h=32, w=32))                                       # 3 * 2^30 input elements
    assert rc == -3 and '2^31' in msg, (rc, msg)
    rc, msg = call(desc(out_h=1 << 14, out_w=64), batch=1 << 10)                      # 3 * 2^30 output elements
    assert rc == -3 and '2^31' in msg, (rc, msg)
    rc, msg = call(desc(n=1, c=1, h=1, w=1 << 30, out_h=1, out_w=1, normalize=0), batch=1)
    assert rc == -3 and 'coefficients' in msg, (rc, msg)
    for std in ((0.2, 0.0, 0.2), (0.2, 0.2, -1.0), (float('nan'), 0.2, 0.2)):
        rc, msg = call(desc(std=std))
        assert rc == -9 and 'std' in msg, (std, rc, msg)                              # NODE_ERR_ARG
    assert issubclass(_lib.NodeHipUnsupported, NotImplementedError) and issubclass(_lib.NodeHipUnsupported, _lib.NodeHipError)
    call(desc(c=2))
    with pytest.raises(NotImplementedError, match='UNSUPPORTED'):
        _lib.check(-3)
    with pytest.raises(_lib.NodeHipError, match='NODE_ERR_ARG') as info:
        _lib.check(-9)
    assert not isinstance(info.value, NotImplementedError)


def test_descriptor_layout_matches_the_header(tmp_path):
    import subprocess
    from neural_ode_features_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ['n', 'c', 'h', 'w', 'out_h', 'out_w', 'normalize', 'mean', 'std']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(node_resize));']
    lines += ['  printf("%s %%zu\\n", offsetof(node_resize, %s));' % (f, f) for f in fields]
    lines += ['  printf("abi %d\\n", NODE_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / 'resize.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'resize'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['size']) == C.sizeof(_lib.NodeResize)
    for f in fields:
        assert int(got[f]) == getattr(_lib.NodeResize, f).offset, f
    assert int(got['abi']) == _lib.NODE_ABI_VERSION == 6              # an addition: the version stays


def test_transfer_transform_arguments():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import augment as A
    assert nof.TransferTransform is A.TransferTransform
    tt = nof.TransferTransform(64, dataset='tiny-imagenet-200')
    assert tt.size == (64, 64) and (tt.mean, tt.std) == A.PREPROC['tiny-imagenet-200']
    d = tt.descriptor((10000, 3, 32, 32))
    assert (d.n, d.c, d.h, d.w, d.out_h, d.out_w, d.normalize) == (10000, 3, 32, 32, 64, 64, 1)
    assert np.allclose(list(d.mean), A.PREPROC['tiny-imagenet-200'][0], atol=1e-7) and np.allclose(list(d.std), A.PREPROC['tiny-imagenet-200'][1], atol=1e-7)
    plain = nof.TransferTransform((9, 50))
    assert plain.size == (9, 50) and plain.mean is None and plain.descriptor((4, 3, 20, 36)).normalize == 0
    assert nof.TransferTransform([48, 40], mean=(0.5,), std=(0.25,)).descriptor((4, 1, 64, 64)).out_w == 40
    for bad in (0, -3, 2.5, True, (32,), (32, 0), (32, 32, 32), '64', None):
        with pytest.raises(ValueError, match='size'):
            nof.TransferTransform(bad)
    with pytest.raises(ValueError, match='known dataset'):
        nof.TransferTransform(64, dataset='imagenet')
    with pytest.raises(ValueError, match='come together'):
        nof.TransferTransform(64, mean=(0.5,))
    with pytest.raises(ValueError, match='std > 0'):
        nof.TransferTransform(64, mean=(0.5, 0.5, 0.5), std=(0.5, 0.0, 0.5))
    with pytest.raises(ValueError, match='3-channel statistics'):
        tt.descriptor((10, 1, 28, 28))
    x, y = torch.zeros(4, 3, 32, 32, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    for call in (tt.batch, tt.resized):
        with pytest.raises(TypeError, match='DeviceSplit'):
            call((x, y), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU path'):
        nof.DeviceSplit(x, y, 'cpu')
    with pytest.raises(TypeError, match='uint8'):
        nof.DeviceSplit(x.float(), y, 'cuda')

    class _Split(nof.DeviceSplit):              # a split without a device: the checks of `index` come before the first HIP call
        def __init__(self):
            self.x, self.y, self.device = x, y, torch.device('cuda', 0)
    for call in (tt.batch, tt.resized):
        with pytest.raises(TypeError, match='int64'):
            call(_Split(), torch.zeros(2, dtype=torch.int32))
        with pytest.raises(TypeError, match='int64'):
            call(_Split(), torch.zeros(2, 1, dtype=torch.int64))
        with pytest.raises(RuntimeError, match='no CPU path'):
            call(_Split(), torch.zeros(2, dtype=torch.int64))


def test_evaluate_parser_and_file_checks(tmp_path):
    from neural_ode_features_amd import evaluate as E
    for mode in ('features', 'retrieval', 'finetune'):
        assert E.parse_args([mode, 'run']).data is None
        with pytest.raises(SystemExit):
            E.parse_args([mode, 'run', '-d', 'imagenet'])
    with pytest.raises(SystemExit, match='--data-file'):
        E.parse_args(['features', 'run', '-d', 'tiny-imagenet-200'])
    with pytest.raises(SystemExit, match='-d/--data'):
        E.parse_args(['features', 'run', '--data-file', 'x.pt'])
    for mode in ('nfe', 'tradeoff', 'accuracy'):
        with pytest.raises(SystemExit, match='features, retrieval and finetune'):
            E.parse_args([mode, 'run', '-d', 'cifar10', '--data-file', 'x.pt'])
    args = E.parse_args(['features', 'run', '--data', 'cifar10', '--data-file', 'x.pt'])
    assert (args.data, args.data_file) == ('cifar10', 'x.pt')
    assert E.parse_args(['retrieval', 'run', '-d', 'cifar10']).data == 'cifar10'          # reads features-cifar10.npz: no file needed
    assert E.result_name('features.npz', None) == 'features.npz' and E.result_name('features.npz', 'cifar10') == 'features-cifar10.npz'
    assert E.result_name('finetune.csv', 'tiny-imagenet-200') == 'finetune-tiny-imagenet-200.csv'
    assert E.result_name('svms', 'tiny-imagenet-200') == 'svms-tiny-imagenet-200'
    # the file's checks need no device
    with pytest.raises(SystemExit, match='not found'):
        E.load_transfer_file(str(tmp_path / 'none.pt'), 3)
    path = str(tmp_path / 'float.pt')
    torch.save({'x_test': torch.zeros(6, 3, 64, 64), 'y_test': torch.zeros(6, dtype=torch.int64)}, path)
    with pytest.raises(SystemExit, match='uint8'):
        E.load_transfer_file(path, 3)
    torch.save({'x_test': torch.zeros(6, 3, 64, 64, dtype=torch.uint8), 'y_test': torch.zeros(6, dtype=torch.int64)}, path)
    with pytest.raises(SystemExit, match='1-channel'):
        E.load_transfer_file(path, 1)
    x, y = E.load_transfer_file(path, 3)
    assert x.shape == (6, 3, 64, 64) and y.shape == (6,)
    torch.save({'x_train': torch.zeros(6, 3, 64, 64, dtype=torch.uint8)}, path)
    with pytest.raises(SystemExit, match='x_test'):
        E.load_transfer_file(path, 3)
    with pytest.raises(SystemExit, match='features-cifar10.npz'):     # (retrieval asks for the device first)
        E.main(['finetune', str(tmp_path), '-d', 'cifar10'])

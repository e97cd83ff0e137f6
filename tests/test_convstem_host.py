"""Host side (no GPU) of the `convolution` stem and of the `ode2` stem's hand-off: state_dict keys, the CPU path of the new
modules, and the argument checks of the C ABI (node_stem_conv's 4x4 geometry, node_downconv_*, node_convstem_*)."""
import ctypes as C
import os
import subprocess

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_ERR_NULL = -1


def _golden(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location='cpu', weights_only=False)


def test_state_dict_keys_are_the_references(golden_dir):
    """The stems of `ODENet(downsample='convolution')` and `'ode2'` keep the keys of the reference's modules: those of the
    fixtures written from `ConvDownsample` and `ODEDownsample2.norm / .conv2`."""
    import neural_ode_features_amd as nof
    conv = nof.ODENet(1, n_filters=64, downsample='convolution')
    assert isinstance(conv.downsample.module, nof.ConvStem) and isinstance(conv.downsample.module, nn.Sequential)
    assert list(conv.downsample.state_dict()) == list(_golden(golden_dir, 'stem_convolution_c64.pt')['state_dict'])
    assert [k for k in conv.state_dict() if k.startswith('downsample.')] == \
        ['downsample.module.%d.%s' % (i, s) for i in (0, 1, 3, 4, 6) for s in ('weight', 'bias')]
    g = _golden(golden_dir, 'ode2_handoff_c64.pt')
    ode2 = nof.ODENet(1, n_filters=64, downsample='ode2')
    keys = list(ode2.state_dict())
    for k in ['downsample.norm.' + k for k in g['norm']] + ['downsample.conv2.' + k for k in g['conv2']]:
        assert k in keys, k
    assert list(g['norm']) == ['0.weight', '0.bias'] and list(g['conv2']) == ['weight', 'bias']
    assert isinstance(nof.ResNet(3, n_filters=64, downsample='convolution').downsample.module, nof.ConvStem)
    assert not isinstance(nof.ODENet(3, n_filters=64, downsample='minimal').downsample.module, nof.ConvStem)


def test_cpu_results_are_the_module_sequences(golden_dir):
    """On the CPU both run the plain modules: the same bits as the module sequence, with the hand-off switch on and off, for the
    last state and for a trajectory."""
    import neural_ode_features_amd as nof
    torch.manual_seed(3)
    stem = nof.ODENet(3, n_filters=64, downsample='convolution').downsample.module
    x = torch.randn(2, 3, 32, 32)
    assert torch.equal(stem(x), nn.Sequential.forward(stem, x))
    assert type(stem(x).grad_fn).__name__ != '_ConvStemFnBackward'

    g = _golden(golden_dir, 'ode2_handoff_c64.pt')
    ode2 = nof.ODEDownsample2(1, 64)
    ode2.norm.load_state_dict(g['norm'])
    ode2.conv2.load_state_dict(g['conv2'])
    plain = lambda t: ode2.conv2(ode2.norm(t.clone()))
    want = plain(g['x'])
    assert torch.allclose(want, g['out'], rtol=1e-4, atol=1e-5)   # the reference's own numbers: same modules
    traj = torch.stack([g['x'], 0.5 * g['x'], g['x'] + 1.0])
    for fused in (True, False):
        ode2.fused_handoff = fused
        assert torch.equal(ode2._handoff(g['x']), want)
        ode2.odeblock.forward = lambda t: g['x']
        ode2.conv1.forward = lambda t: t
        assert torch.equal(ode2(g['x']), want)
        ode2.odeblock.forward = lambda t: traj
        for apply_conv in (True, False):
            ode2.apply_conv = apply_conv
            first, last = ode2(g['x'])
            assert torch.equal(last, plain(traj[-1]))
            per_slice = torch.stack([ode2.norm(t.clone()) for t in traj])
            if apply_conv:
                per_slice = torch.stack([ode2.conv2(t) for t in per_slice])
            assert torch.equal(first, per_slice)


def test_conv4_geometry_is_the_only_new_one():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    size = lambda *g: lib.node_stem_conv_workspace_bytes(C.byref(_lib.NodeConvGeom(*g)))
    assert size(8, 64, 64, 30, 30, 4, 2, 1) > 0
    assert size(8, 256, 256, 16, 16, 4, 2, 1) > size(8, 64, 64, 16, 16, 4, 2, 1) > 0
    for bad, word in (((8, 64, 64, 30, 30, 4, 1, 1), 'stride'), ((8, 64, 64, 30, 30, 4, 2, 0), 'pad'),
                      ((8, 24, 64, 30, 30, 4, 2, 1), '64'), ((8, 64, 64, 30, 30, 4, 2, 2), 'pad'), ((8, 64, 64, 3, 30, 4, 2, 1), '4x4'),
                      ((8, 64, 64, 30, 30, 5, 2, 1), '3x3'), ((8, 64, 64, 30, 30, 2, 2, 1), '3x3')):
        assert size(*bad) == 0, bad
        assert word in lib.node_last_error().decode(), (bad, lib.node_last_error())
    assert size(8, 64, 64, 30, 30, 3, 2, 1) > 0 and size(8, 64, 64, 30, 30, 1, 2, 0) > 0          # as before


def test_downconv_entry_points_host_side():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeDownConvShape
    size = lambda sh, keep=1: lib.node_downconv_workspace_bytes(C.byref(sh), keep)
    cifar, mnist = S(128, 256, 256, 16, 16, 1e-5), S(32, 64, 64, 14, 14, 1e-5)
    assert 0 < size(mnist) < size(cifar) < (2 << 30)
    assert 0 < size(cifar, 0) < size(cifar)                       # the forward alone needs less
    assert size(S(21 * 128, 256, 256, 16, 16, 1e-5), 0) > 0       # a 21-slice trajectory as one batch
    for bad, word in ((S(8, 24, 24, 14, 14, 1e-5), 'filters'), (S(8, 64, 24, 14, 14, 1e-5), 'filters'), (S(8, 192, 192, 14, 14, 1e-5), 'filters'),
                      (S(8, 64, 64, 64, 64, 1e-5), 'LDS'), (S(0, 64, 64, 14, 14, 1e-5), 'shape'), (S(8, 64, 64, 3, 14, 1e-5), 'shape'),
                      (S(1 << 14, 256, 256, 32, 32, 1e-5), '2^31')):
        assert size(bad) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
    assert lib.node_downconv_workspace_bytes(None, 1) == 0
    assert lib.node_downconv_fwd(None, None, None, None, 1, None, 0, None) == NODE_ERR_NULL
    assert lib.node_downconv_fwd(C.byref(mnist), None, None, None, 1, None, 0, None) == NODE_ERR_NULL
    assert lib.node_downconv_bwd(C.byref(mnist), None, None, None, None, None, 0, None) == NODE_ERR_NULL
    assert lib.node_downconv_fwd(C.byref(S(8, 24, 24, 14, 14, 1e-5)), None, None, None, 1, None, 0, None) == _lib.NODE_ERR_UNSUPPORTED


def test_convstem_entry_points_host_side():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeConvStemShape
    size = lambda sh, keep=1: lib.node_convstem_workspace_bytes(C.byref(sh), keep)
    cifar, mnist = S(128, 3, 32, 32, 256, 1e-5), S(32, 1, 28, 28, 64, 1e-5)
    assert 0 < size(mnist) < size(cifar) < (2 << 30)
    assert 0 < size(cifar, 0) < size(cifar)
    for bad, word in ((S(8, 4, 32, 32, 64, 1e-5), 'in_ch'), (S(8, 3, 32, 32, 24, 1e-5), 'filters'), (S(8, 3, 32, 32, 192, 1e-5), 'filters'),
                      (S(8, 3, 64, 64, 64, 1e-5), 'LDS'), (S(0, 3, 32, 32, 64, 1e-5), 'shape'), (S(8, 3, 8, 32, 64, 1e-5), 'shape')):
        assert size(bad) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
    assert lib.node_convstem_workspace_bytes(None, 1) == 0
    assert lib.node_convstem_fwd(None, None, None, None, 1, None, 0, None) == NODE_ERR_NULL
    assert lib.node_convstem_fwd(C.byref(mnist), None, None, None, 1, None, 0, None) == NODE_ERR_NULL
    assert lib.node_convstem_bwd(C.byref(mnist), None, None, None, None, None, 0, None) == NODE_ERR_NULL


def test_ctypes_layouts_of_the_new_structs_match_the_header(tmp_path):
    """tests/test_host_and_abi.py::test_header_is_plain_c_and_ctypes_layouts_match for the structs this ABI addition brings."""
    from neural_ode_features_amd import _lib
    structs = {
        'node_downconv_shape': (_lib.NodeDownConvShape, ['n', 'cin', 'cout', 'h', 'w', 'eps']),
        'node_downconv_params': (_lib.NodeDownConvParams, list(_lib.DOWNCONV_PARAM_FIELDS)),
        'node_downconv_grads': (_lib.NodeDownConvParams, list(_lib.DOWNCONV_PARAM_FIELDS)),
        'node_convstem_shape': (_lib.NodeConvStemShape, ['n', 'in_ch', 'h', 'w', 'filters', 'eps']),
        'node_convstem_params': (_lib.NodeConvStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
        'node_convstem_grads': (_lib.NodeConvStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
        'node_conv_geom': (_lib.NodeConvGeom, ['n', 'cin', 'cout', 'x_h', 'x_w', 'k', 'stride', 'pad']),
    }
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {']
    for name, (_, fields) in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    lines += ['  return 0;', '}']
    src = tmp_path / 'abi.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, (ct, fields) in structs.items():
        assert int(got[name]) == C.sizeof(ct), name
        for f in fields:
            assert int(got['%s.%s' % (name, f)]) == getattr(ct, f).offset, (name, f)
    for name in ('node_downconv_workspace_bytes', 'node_downconv_fwd', 'node_downconv_bwd',
                 'node_convstem_workspace_bytes', 'node_convstem_fwd', 'node_convstem_bwd'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)

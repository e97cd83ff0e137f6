"""Host side (no GPU) of the `minimal` stem and of the conv stems' input gradients: state_dict keys, the CPU path of
`MinimalStem`, the `input_grad` switches and `attack._frozen`, and the argument checks of the C ABI (node_ministem_*,
node_convstem_bwd_dx)."""
import ctypes as C
import os
import subprocess

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_ERR_NULL = -1


def _golden(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location='cpu', weights_only=False)


def test_state_dict_keys_are_the_references(golden_dir):
    """The stem of `ODENet` / `ResNet` with `downsample='minimal'` keeps the keys of the reference's `MinimalConvDownsample`
    (the fixture's), and it is a `MinimalStem`, which is no `ConvStem`."""
    import neural_ode_features_amd as nof
    want = list(_golden(golden_dir, 'stem_minimal_c64.pt')['state_dict'])
    assert want == ['module.%d.%s' % (i, s) for i in (0, 1, 3, 4, 6) for s in ('weight', 'bias')]
    for net in (nof.ODENet(1, n_filters=64, downsample='minimal'), nof.ResNet(1, n_filters=64, downsample='minimal')):
        stem = net.downsample.module
        assert isinstance(stem, nof.MinimalStem) and isinstance(stem, nn.Sequential) and not isinstance(stem, nof.ConvStem)
        assert list(net.downsample.state_dict()) == want
        assert [k for k in net.state_dict() if k.startswith('downsample.')] == ['downsample.' + k for k in want]
        assert stem[0].out_channels == 24 and stem[1].num_groups == 24 and stem[6].out_channels == 64
    assert not issubclass(nof.MinimalStem, nof.ConvStem) and not issubclass(nof.ConvStem, nof.MinimalStem)


@pytest.mark.parametrize('kind', ['minimal', 'convolution'])
def test_cpu_results_are_the_module_sequences(kind):
    """On the CPU the stem runs the plain modules: the same bits as `nn.Sequential.forward`, with either switch setting, for an
    input with and without a gradient; the input gradient is the module sequence's."""
    import neural_ode_features_amd as nof
    torch.manual_seed(3)
    stem = nof.ODENet(3, n_filters=64, downsample=kind).downsample.module
    assert type(stem).input_grad is False
    x = torch.randn(2, 3, 32, 32)
    for on in (False, True):
        stem.input_grad = on
        out = stem(x)
        assert torch.equal(out, nn.Sequential.forward(stem, x))
        assert 'StemFn' not in type(out.grad_fn).__name__
        xg = x.clone().requires_grad_(True)
        stem(xg).sum().backward()
        xr = x.clone().requires_grad_(True)
        nn.Sequential.forward(stem, xr).sum().backward()
        assert torch.equal(xg.grad, xr.grad)
        assert torch.equal(stem(x.double().float()), out)


def test_batch_norm_builds_and_runs_the_module_sequence():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import ministem
    torch.manual_seed(5)
    stem = nof.ODENet(3, n_filters=64, downsample='minimal', norm='batch').downsample.module
    assert isinstance(stem, nof.MinimalStem) and isinstance(stem[1], nn.BatchNorm2d)
    assert ministem._params_of(stem) is None       # not the layout the kernels take: never fused, on any device
    x = torch.randn(4, 3, 32, 32)
    stem.eval()
    assert torch.equal(stem(x), nn.Sequential.forward(stem, x))
    assert ministem._params_of(nof.ODENet(3, n_filters=64, downsample='minimal').downsample.module) is not None


def test_frozen_switches_input_grad_on_all_three_stems_and_restores():
    """`attack._frozen`: `input_grad` on for `ResidualStem`, `ConvStem` and `MinimalStem` instances and parameters without
    gradients for the duration; both restored afterwards, also when the body raises."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import attack
    from neural_ode_features_amd.stem import ResidualStem
    nets = [nof.ResNet(3, n_filters=64, downsample=k) for k in ('residual', 'convolution', 'minimal')]
    model = nn.ModuleList(nets)
    stems = [n.downsample.module for n in nets]
    assert [type(s) for s in stems] == [ResidualStem, nof.ConvStem, nof.MinimalStem]
    stems[1].input_grad = True            # one that was already on stays on afterwards
    before = [s.input_grad for s in stems]
    with attack._frozen(model, True):
        assert all(s.input_grad is True for s in stems)
        assert not any(p.requires_grad for p in model.parameters())
    assert [s.input_grad for s in stems] == before and all(p.requires_grad for p in model.parameters())
    with attack._frozen(model, False):
        assert not any(s.input_grad for s in stems)
    assert [s.input_grad for s in stems] == before
    with pytest.raises(KeyError):
        with attack._frozen(model, True):
            assert all(s.input_grad is True for s in stems)
            raise KeyError('the body fails')
    assert [s.input_grad for s in stems] == before and all(p.requires_grad for p in model.parameters())


def test_ministem_entry_points_host_side():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeMiniStemShape
    size = lambda sh, keep=1: lib.node_ministem_workspace_bytes(C.byref(sh), keep)
    cifar, mnist = S(128, 3, 32, 32, 256, 1e-5), S(32, 1, 28, 28, 64, 1e-5)
    assert 0 < size(mnist) < size(cifar) < (1 << 30)
    assert 0 < size(cifar, 0) < size(cifar)                       # the forward alone needs less
    assert size(S(2, 3, 10, 10, 64, 1e-5)) > 0 and size(S(2, 3, 64, 64, 4096, 1e-5)) > 0
    for bad, word in ((S(8, 4, 32, 32, 64, 1e-5), 'in_ch'), (S(8, 3, 32, 32, 24, 1e-5), 'filters'), (S(8, 3, 32, 32, 192, 1e-5), 'filters'),
                      (S(8, 3, 32, 32, 8192, 1e-5), 'filters'), (S(0, 3, 32, 32, 64, 1e-5), 'shape'), (S(8, 3, 8, 32, 64, 1e-5), '10 x 10'),
                      (S(8, 3, 32, 9, 64, 1e-5), '10 x 10'), (S(1 << 16, 3, 64, 64, 64, 1e-5), '2^31')):
        assert size(bad) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
    assert lib.node_ministem_workspace_bytes(None, 1) == 0
    assert lib.node_ministem_fwd(None, None, None, None, 1, None, 0, None) == NODE_ERR_NULL
    assert lib.node_ministem_fwd(C.byref(mnist), None, None, None, 1, None, 0, None) == NODE_ERR_NULL
    assert lib.node_ministem_bwd(None, None, None, None, None, None, None, 0, None) == NODE_ERR_NULL
    assert lib.node_ministem_bwd(C.byref(mnist), None, None, None, None, None, None, 0, None) == NODE_ERR_NULL
    assert lib.node_ministem_fwd(C.byref(S(8, 3, 32, 32, 192, 1e-5)), None, None, None, 1, None, 0, None) == _lib.NODE_ERR_UNSUPPORTED
    # every pointer but grads and d_x given (host addresses: nothing is launched before the check): both NULL is refused by name
    buf = (C.c_float * 64)()
    addr = C.addressof(buf)
    prm = _lib.NodeMiniStemParams(*[addr] * 10)
    rc = lib.node_ministem_bwd(C.byref(mnist), C.byref(prm), addr, addr, None, None, 256, size(mnist), None)
    assert rc == NODE_ERR_NULL and b'both NULL' in lib.node_last_error()


def test_convstem_bwd_dx_host_side():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeConvStemShape
    mnist = S(32, 1, 28, 28, 64, 1e-5)
    assert lib.node_convstem_bwd_dx(None, None, None, None, None, None, None, 0, None) == NODE_ERR_NULL
    assert lib.node_convstem_bwd_dx(C.byref(mnist), None, None, None, None, None, None, 0, None) == NODE_ERR_NULL
    buf = (C.c_float * 64)()
    addr = C.addressof(buf)
    prm = _lib.NodeConvStemParams(*[addr] * 10)
    nbytes = lib.node_convstem_workspace_bytes(C.byref(mnist), 1)
    # d_x is required, with or without grads
    assert lib.node_convstem_bwd_dx(C.byref(mnist), C.byref(prm), addr, addr, C.byref(prm), None, 256, nbytes, None) == NODE_ERR_NULL
    assert lib.node_convstem_bwd_dx(C.byref(mnist), C.byref(prm), addr, addr, None, None, 256, nbytes, None) == NODE_ERR_NULL
    # node_convstem_bwd still requires grads; the refusals are the forward's
    assert lib.node_convstem_bwd(C.byref(mnist), C.byref(prm), addr, addr, None, 256, nbytes, None) == NODE_ERR_NULL
    for bad, word in ((S(8, 3, 32, 32, 24, 1e-5), 'filters'), (S(8, 3, 64, 64, 64, 1e-5), 'LDS')):
        assert lib.node_convstem_bwd_dx(C.byref(bad), C.byref(prm), addr, addr, None, addr, 256, nbytes, None) == _lib.NODE_ERR_UNSUPPORTED
        assert word in lib.node_last_error().decode()
    # a workspace that is too small is refused before anything is launched
    assert lib.node_convstem_bwd_dx(C.byref(mnist), C.byref(prm), addr, addr, None, addr, 256, 1024, None) == -4


def test_ctypes_layouts_of_the_new_structs_match_the_header(tmp_path):
    """The gcc `offsetof` program of tests/test_convstem_host.py for the structs this ABI addition brings; the version stays 6."""
    from neural_ode_features_amd import _lib
    structs = {
        'node_ministem_shape': (_lib.NodeMiniStemShape, ['n', 'in_ch', 'h', 'w', 'filters', 'eps']),
        'node_ministem_params': (_lib.NodeMiniStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
        'node_ministem_grads': (_lib.NodeMiniStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
    }
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {']
    for name, (_, fields) in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    lines += ['  printf("abi %d\\n", NODE_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / 'abi.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, (ct, fields) in structs.items():
        assert int(got[name]) == C.sizeof(ct), name
        for f in fields:
            assert int(got['%s.%s' % (name, f)]) == getattr(ct, f).offset, (name, f)
    lib = _lib.load()
    for name in ('node_ministem_workspace_bytes', 'node_ministem_fwd', 'node_ministem_bwd', 'node_convstem_bwd_dx'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert int(got['abi']) == 6 == _lib.NODE_ABI_VERSION == lib.node_abi_version()

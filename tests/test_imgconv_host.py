"""The image convolution in front of the ODE block (include/node_hip.h: node_imgconv_*; neural_ode_features_amd/imgconv.py), as far
as it goes without a GPU: exports, argument checks before any device call, the ctypes twin of the shape struct, unchanged
state_dict keys, and the parent path for everything the kernels do not take."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in ('node_imgconv_workspace_bytes', 'node_imgconv_fwd', 'node_imgconv_bwd'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_argument_checks_need_no_gpu():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeImgConvShape
    p = 4096                                  # an address no check dereferences
    assert lib.node_imgconv_fwd(None, p, p, p, p, None) == -1                       # NODE_ERR_NULL
    assert lib.node_imgconv_bwd(None, p, p, p, p, p, p, p, 1 << 30, None) == -1
    good = S(8, 3, 32, 32, 64)
    assert lib.node_imgconv_fwd(C.byref(good), None, p, p, p, None) == -1
    assert lib.node_imgconv_fwd(C.byref(good), p, p, None, None, None) == -1        # bias may be NULL, y may not
    assert lib.node_imgconv_bwd(C.byref(good), p, p, p, None, p, p, p, 1 << 30, None) == -1
    for bad, word in ((S(8, 3, 32, 32, 48), 'filters'), (S(8, 5, 32, 32, 64), 'in_ch'), (S(8, 3, 31, 32, 64), 'h=31'),
                      (S(8, 3, 32, 2, 64), 'w=2'), (S(8, 0, 32, 32, 64), 'in_ch')):
        assert lib.node_imgconv_workspace_bytes(C.byref(bad)) == 0
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_imgconv_fwd(C.byref(bad), p, p, p, p, None) == -3           # NODE_ERR_UNSUPPORTED
        assert word in lib.node_last_error().decode()
        assert lib.node_imgconv_bwd(C.byref(bad), p, p, p, p, p, p, p, 1 << 30, None) == -3
    assert lib.node_imgconv_workspace_bytes(C.byref(S(0, 3, 32, 32, 64))) == 0
    cifar = lib.node_imgconv_workspace_bytes(C.byref(S(128, 3, 32, 32, 256)))
    mnist = lib.node_imgconv_workspace_bytes(C.byref(S(128, 1, 28, 28, 64)))
    assert 0 < mnist < cifar < (64 << 20)
    shape = S(128, 3, 32, 32, 256)
    assert lib.node_imgconv_bwd(C.byref(shape), p, p, p, p, p, p, p, cifar - 1, None) == -4     # NODE_ERR_WORKSPACE
    assert b'workspace too small' in lib.node_last_error()
    assert lib.node_imgconv_bwd(C.byref(shape), p, p, p, p, p, p, None, cifar, None) == -4
    assert lib.node_imgconv_bwd(C.byref(shape), p, p, p, p, p, p + 4, p, cifar, None) == -9     # d_x is stored as float2


def test_shape_struct_matches_its_ctypes_twin(tmp_path):
    from neural_ode_features_amd import _lib
    fields = ['n', 'in_ch', 'h', 'w', 'filters']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(node_imgconv_shape));']
    lines += ['  printf("%s %%zu\\n", offsetof(node_imgconv_shape, %s));' % (f, f) for f in fields]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'abi.c', tmp_path / 'abi'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['size']) == C.sizeof(_lib.NodeImgConvShape)
    for f in fields:
        assert int(got[f]) == getattr(_lib.NodeImgConvShape, f).offset, f


@pytest.mark.parametrize('kind', ['one-shot', 'ode', 'ode2'])
def test_state_dict_keys_are_those_of_plain_conv2d(kind, monkeypatch):
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import odenet
    torch.manual_seed(0)
    net = nof.ODENet(3, downsample=kind)
    prefix = 'downsample.module.' if kind == 'one-shot' else 'downsample.conv1.'
    conv = net.downsample.module if kind == 'one-shot' else net.downsample.conv1
    assert isinstance(conv, nof.ImageConv2d) and isinstance(conv, nn.Conv2d)
    keys = list(net.state_dict().keys())
    assert [k for k in keys if k.startswith(prefix)] == [prefix + 'weight', prefix + 'bias']
    if kind == 'one-shot':
        assert [k for k in keys if k.startswith('downsample.')] == [prefix + 'weight', prefix + 'bias']
    # the same net built from plain nn.Conv2d modules: same keys in the same order, same initial values, and its state_dict loads
    monkeypatch.setattr(odenet, 'ImageConv2d', nn.Conv2d)
    torch.manual_seed(0)
    plain = nof.ODENet(3, downsample=kind)
    pconv = plain.downsample.module if kind == 'one-shot' else plain.downsample.conv1
    assert type(pconv) is nn.Conv2d
    sd = plain.state_dict()
    assert list(sd.keys()) == keys
    for k in keys:
        assert torch.equal(sd[k], net.state_dict()[k]), k
    with torch.no_grad():
        pconv.weight.add_(1.0)
    net.load_state_dict(plain.state_dict(), strict=True)
    assert torch.equal(conv.weight, pconv.weight)


def test_cpu_tensors_take_the_parent_path_bit_for_bit():
    import neural_ode_features_amd as nof
    torch.manual_seed(1)
    for cin, filters, h, w in ((3, 64, 32, 32), (1, 64, 28, 28), (3, 16, 9, 12)):
        m = nof.ImageConv2d(cin, filters)
        assert (m.kernel_size, m.stride, m.padding) == ((4, 4), (2, 2), (1, 1))
        x = torch.randn(2, cin, h, w, requires_grad=True)
        y = m(x)
        assert torch.equal(y, F.conv2d(x, m.weight, m.bias, 2, 1))
        y.sum().backward()
        assert x.grad is not None and m.weight.grad is not None


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be a CUDA tensor: the device question of `fusable` without a GPU."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def _on_fake_device(m):
    """The module with its parameters replaced by CPU tensors that claim to be CUDA tensors."""
    for name in ('weight', 'bias'):
        t = m._parameters.pop(name)
        setattr(m, name, None if t is None else _FakeCuda(t.detach()))
    return m


def test_fusable_geometry():
    from neural_ode_features_amd import imgconv
    import neural_ode_features_amd as nof
    x = torch.zeros(2, 3, 32, 32)
    fx = _FakeCuda(x)
    assert not imgconv.fusable(nof.ImageConv2d(3, 64), x)                          # CPU tensor
    assert not imgconv.fusable(nof.ImageConv2d(3, 16), x)
    assert not imgconv.fusable(nof.ImageConv2d(3, 64), fx)                         # parameters on the CPU
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64)), x)         # input on the CPU
    # input AND parameters claim a device: what is left is the geometry, and each refusal has its accepted neighbour
    assert imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64)), fx)
    assert imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 256)), fx)
    assert imgconv.fusable(_on_fake_device(nof.ImageConv2d(1, 64, bias=False)), _FakeCuda(torch.zeros(3, 1, 28, 28)))
    assert imgconv.fusable(_on_fake_device(nof.ImageConv2d(4, 128)), _FakeCuda(torch.zeros(1, 4, 4, 6)))
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 16)), fx)        # 16 filters: on no device
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 96)), fx)
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(5, 64)), _FakeCuda(torch.zeros(2, 5, 32, 32)))
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64)), _FakeCuda(torch.zeros(2, 3, 31, 32)))
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64)), _FakeCuda(torch.zeros(2, 3, 32, 2)))
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64)), _FakeCuda(torch.zeros(2, 1, 32, 32)))
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64)), _FakeCuda(torch.zeros(3, 32, 32)))
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64)), _FakeCuda(x.double()))
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64).double()), fx)
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64, 3, 1, 1)), fx)
    assert not imgconv.fusable(_on_fake_device(nof.ImageConv2d(3, 64, 4, 2, 1, padding_mode='reflect')), fx)


def test_filters_have_an_upper_bound():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeImgConvShape
    assert lib.node_imgconv_workspace_bytes(C.byref(S(1, 1, 4, 4, 65536))) > 0
    assert lib.node_imgconv_workspace_bytes(C.byref(S(1, 1, 4, 4, 65536 + 64))) == 0
    assert b'filters' in lib.node_last_error()
    assert lib.node_imgconv_fwd(C.byref(S(1, 1, 4, 4, 1 << 22)), 4096, 4096, 4096, 4096, None) == -3

"""The `ode` stem's hand-off (include/node_hip.h: node_pool_*; neural_ode_features_amd/pool.py) as far as it goes without a GPU:
exports, argument checks before any device call, the ctypes twin of the shape struct, the module path of CPU tensors bit for bit,
unchanged state_dict keys and the trajectory means handed from the stem to `ODENet.forward`."""
import ctypes as C
import os
import subprocess

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in ('node_pool_fwd', 'node_pool_bwd'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.node_abi_version() == 6          # additions only


def test_shape_struct_matches_its_ctypes_twin(tmp_path):
    from neural_ode_features_amd import _lib
    fields = ['t', 'n', 'c', 'h', 'w']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(node_pool_shape));']
    lines += ['  printf("%s %%zu\\n", offsetof(node_pool_shape, %s));' % (f, f) for f in fields]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'abi.c', tmp_path / 'abi'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['size']) == C.sizeof(_lib.NodePoolShape)
    assert [f for f, _ in _lib.NodePoolShape._fields_] == fields
    for f in fields:
        assert int(got[f]) == getattr(_lib.NodePoolShape, f).offset, f


def test_argument_checks_need_no_gpu():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodePoolShape
    p = 4096                                  # an address no check dereferences
    assert lib.node_pool_fwd(None, p, p, p, p, None) == -1                           # NODE_ERR_NULL
    assert lib.node_pool_bwd(None, p, p, p, None) == -1
    good = S(1, 4, 8, 16, 16)
    assert lib.node_pool_fwd(C.byref(good), None, p, None, None, None) == -1
    assert lib.node_pool_fwd(C.byref(good), p, None, None, None, None) == -1         # argmax and means may be NULL, pooled may not
    assert lib.node_pool_bwd(C.byref(good), p, None, p, None) == -1
    assert lib.node_pool_bwd(C.byref(good), p, p, None, None) == -1
    assert lib.node_pool_fwd(C.byref(good), p + 2, p, None, None, None) == -9        # NODE_ERR_ARG: floats
    for bad, word in ((S(0, 4, 8, 16, 16), 't=0'), (S(1, 0, 8, 16, 16), 'n=0'), (S(1, 4, 0, 16, 16), 'c=0'), (S(1, 4, 8, 1, 16), 'h=1'),
                      (S(1, 4, 8, 16, 1), 'w=1'), (S(1, 4, 8, 16, 40000), 'w=40000'), (S(64, 1 << 15, 1 << 15, 1 << 10, 1 << 10), '2^40')):
        assert lib.node_pool_fwd(C.byref(bad), p, p, p, p, None) == -3               # NODE_ERR_UNSUPPORTED
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_pool_bwd(C.byref(bad), p, p, p, None) == -3
        assert word in lib.node_last_error().decode()


def test_cpu_tensors_take_the_module_path_bit_for_bit():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import pool
    torch.manual_seed(3)
    for n, c, h, w in ((3, 16, 16, 16), (2, 5, 7, 7), (1, 3, 5, 9), (2, 8, 2, 2)):
        x = torch.randint(0, 3, (n, c, h, w)).float().requires_grad_(True)
        assert not pool.fusable(x)
        y = nof.max_pool_4s2(x)
        assert type(y.grad_fn).__name__ != '_MaxPool4s2FnBackward'
        ref = F.max_pool2d(x, 4, 2, 1)
        assert torch.equal(y, ref)
        gy = torch.randn(ref.shape)
        assert torch.equal(torch.autograd.grad(y, x, gy)[0], torch.autograd.grad(ref, x, gy)[0])
        traj = torch.randn(4, n, c, h, w) + 100.0
        means, last = nof.trajectory_pool(traj)
        assert means.shape == (4, n, c)
        assert torch.equal(means, torch.stack([f.mean(-1).mean(-1) for f in traj]))
        assert torch.equal(last, F.max_pool2d(traj[-1], 4, 2, 1))
    assert not pool.fusable(torch.zeros(2, 3, 16)) and not pool.fusable(None)


def test_ode_net_keeps_its_keys_and_its_maxpool_module():
    import neural_ode_features_amd as nof
    torch.manual_seed(0)
    net = nof.ODENet(3, n_filters=16, downsample='ode')
    stem = net.downsample
    assert type(stem.maxpool) is nn.MaxPool2d and (stem.maxpool.kernel_size, stem.maxpool.stride, stem.maxpool.padding) == (4, 2, 1)
    assert nof.ODEDownsample.fused_pool is True
    keys = list(net.state_dict().keys())
    assert [k for k in keys if k.startswith('downsample.')] == \
        ['downsample.conv1.weight', 'downsample.conv1.bias'] + ['downsample.odeblock.' + k for k in stem.odeblock.state_dict().keys()]
    assert not any('maxpool' in k or 'pool' in k for k in keys)
    assert keys[-2:] == ['classifier.module.4.weight', 'classifier.module.4.bias']


def test_feature_extraction_on_the_cpu_is_what_it_was(monkeypatch):
    """`ODENet.forward` with an `ode` stem in feature mode, on the CPU (nothing fusable): the features of the plain path with
    `fused_pool` on and off, and the stem's means are the ones `forward` returns when the stem hands some back."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import odenet

    class _Block(nn.Module):                  # stands in for the HIP solve: a two-slice trajectory, or its last slice
        return_last_only = True
        nfe = 0

        def forward(self, x):
            return x + 1.0 if self.return_last_only else torch.stack([x, x + 1.0])

    torch.manual_seed(1)
    net = nof.ODENet(3, n_filters=16, downsample='ode')
    net.downsample.odeblock, net.odeblock = _Block(), _Block()
    x = torch.randn(2, 3, 16, 16)
    y = net(x)
    assert y.shape == (2, 10)
    net.to_features_extractor()
    net.eval()
    with torch.no_grad():
        out = net.downsample(x, with_means=True)
        assert isinstance(out, tuple) and len(out) == 2 and out.means is None          # CPU: the caller pools
        assert torch.equal(out[1], F.max_pool2d(out[0][-1], 4, 2, 1))
        feats = net(x)
        monkeypatch.setattr(odenet.ODEDownsample, 'fused_pool', False)
        assert torch.equal(net(x), feats)
    assert feats.shape == (4, 2, 16)
    assert torch.equal(feats[:2], torch.stack([f.mean(-1).mean(-1) for f in out[0]]))
    # a stem that hands its means back: forward takes them and does not pool the trajectory again
    marked = odenet.StemTrajectory(out)
    marked.means = torch.full((2, 2, 16), 7.0)
    monkeypatch.setattr(net.downsample, 'forward', lambda x, with_means=False: marked)
    with torch.no_grad():
        assert torch.equal(net(x)[:2], marked.means) and torch.equal(net(x)[2:], feats[2:])

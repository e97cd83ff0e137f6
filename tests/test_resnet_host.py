"""No GPU: the ResNet baseline (resnet.py; reference model.py:65-111) against fixtures the reference itself wrote
(tests/golden/make_golden_resnet.py), the host side of the trunk's C ABI (node_trunk_workspace_bytes), the model builder
`train` and `evaluate.load_run` share, and the `--model` flag of the training command line."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_state_dict_keys_and_shapes_are_the_references(golden_dir):
    import neural_ode_features_amd as nof
    want = json.load(open(os.path.join(golden_dir, 'resnet_keys.json')))
    nets = {'resnet_3_f256_residual': nof.ResNet(3, n_filters=256, downsample='residual'),
            'resnet_1_f64_one-shot': nof.ResNet(1, n_filters=64, downsample='one-shot')}
    assert set(want) == set(nets)
    for tag, net in nets.items():
        got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        assert got == want[tag], tag
        assert isinstance(net.features, nof.ResidualTrunk) and len(net.features) == 6


def test_reference_fixture_on_the_cpu(golden_dir):
    """tests/golden/resnet_oneshot_c16.pt: strict load, then logits, loss, every gradient and both feature-extractor outputs.
    Both sides are fp32 PyTorch running the same operators (1e-5 of max|ref|); an error of semantics is O(1)."""
    import copy
    import neural_ode_features_amd as nof
    g = torch.load(os.path.join(golden_dir, 'resnet_oneshot_c16.pt'), map_location='cpu', weights_only=False)
    net = nof.ResNet(1, out=10, n_filters=16, downsample='one-shot')
    net.load_state_dict(g['state_dict'], strict=True)
    assert net.nfe() == 0 and net.nfe(reset=True) == 0
    net.eval()
    with torch.no_grad():
        logits = net(g['x'])
    assert _rel(logits, g['logits']) <= 1e-5
    net.train()
    loss = F.cross_entropy(net(g['x']), g['y'])
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) <= 1e-5 * abs(float(g['loss']))
    grads = dict(net.named_parameters())
    assert set(grads) == set(g['grads'])
    for name, ref in g['grads'].items():
        assert _rel(grads[name].grad, ref) <= 1e-5, name
    pooled = copy.deepcopy(net).eval()
    pooled.to_features_extractor()
    with torch.no_grad():
        feats = pooled(g['x'])
    assert tuple(feats.shape) == (7, 3, 16)
    assert _rel(feats, g['features']) <= 1e-5
    unpooled = copy.deepcopy(net).eval()
    unpooled.to_features_extractor(keep_pool=False)
    with torch.no_grad():
        full = unpooled(g['x'])
    assert list(full.shape) == g['features_nopool_shape'] == [7, 3, 16, 14, 14]


def test_batch_norm_builds_the_module_sequence():
    import neural_ode_features_amd as nof
    net = nof.ResNet(3, n_filters=16, downsample='one-shot', norm='batch')
    assert isinstance(net.features[0].norm1, torch.nn.BatchNorm2d)
    assert net(torch.randn(2, 3, 8, 8)).shape == (2, 10)
    with pytest.raises(NotImplementedError):
        nof.ResNet(3, downsample='ode')


def test_trunk_workspace_bytes_host_side():
    from neural_ode_features_amd import _lib
    lib = _lib.load()

    def nbytes(n, c, h, w, blocks, keep):
        return lib.node_trunk_workspace_bytes(C.byref(_lib.NodeTrunkShape(n, c, h, w, blocks, 1e-5)), keep)

    for n, c, h, w in ((128, 256, 8, 8), (128, 64, 7, 7), (128, 64, 14, 14), (128, 256, 16, 16)):
        keep, scratch = nbytes(n, c, h, w, 6, 1), nbytes(n, c, h, w, 6, 0)
        assert 0 < scratch < keep < (4 << 30), (n, c, h, w, scratch, keep)
    for bad, word in (((8, 96, 8, 8, 6), 'channels'), ((8, 32, 8, 8, 6), 'channels'), ((8, 64, 8, 8, 0), 'blocks'),
                      ((0, 64, 8, 8, 6), 'shape'), ((8, 64, 64, 64, 6), 'LDS')):
        assert nbytes(*bad, 1) == 0, bad
        assert word in lib.node_last_error().decode(), (bad, lib.node_last_error())
    assert lib.node_trunk_workspace_bytes(None, 1) == 0
    assert 'NULL' in lib.node_last_error().decode()
    # the calls themselves refuse the same shapes, and a missing pointer, before anything touches a device
    shape = _lib.NodeTrunkShape(8, 96, 8, 8, 6, 1e-5)
    assert lib.node_trunk_fwd(C.byref(shape), None, None, None, None, 1, None, 0, None) == -3
    shape = _lib.NodeTrunkShape(8, 64, 8, 8, 6, 1e-5)
    assert lib.node_trunk_fwd(C.byref(shape), None, None, None, None, 1, None, 0, None) == -1
    assert lib.node_trunk_bwd(C.byref(shape), None, None, None, None, None, 0, None) == -1


def test_ctypes_layouts_of_the_trunk_structs(tmp_path):
    import subprocess
    from neural_ode_features_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {'node_trunk_shape': (_lib.NodeTrunkShape, ['n', 'channels', 'h', 'w', 'blocks', 'eps']),
               'node_trunk_block': (_lib.NodeTrunkBlock, list(_lib.TRUNK_BLOCK_FIELDS)),
               'node_trunk_block_grads': (_lib.NodeTrunkBlock, list(_lib.TRUNK_BLOCK_FIELDS))}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {']
    for name, (_, fields) in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / 'abi.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, (ct, fields) in structs.items():
        assert int(got[name]) == C.sizeof(ct), name
        for f in fields:
            assert int(got['%s.%s' % (name, f)]) == getattr(ct, f).offset, (name, f)


def test_shared_model_builder():
    import types
    import neural_ode_features_amd as nof
    base = dict(filters=16, downsample='one-shot', dropout=0, norm='group', method='rk4', tol=1e-2, adjoint=True)
    net = nof.build_model(dict(base, model='resnet'), 1, 10)
    assert isinstance(net, nof.ResNet) and net.classifier.module[-1].out_features == 10
    for params in (dict(base), dict(base, model='odenet'), types.SimpleNamespace(**base)):
        net = nof.build_model(params, 3, 7)
        assert isinstance(net, nof.ODENet) and net.odeblock.method == 'rk4' and net.odeblock.tol == 1e-2
    assert isinstance(nof.build_model(types.SimpleNamespace(model='resnet', **base), 3, 7), nof.ResNet)
    with pytest.raises(ValueError):
        nof.build_model(dict(base, model='vgg'), 1, 10)


def test_train_parser_model_flag_and_run_directory():
    from neural_ode_features_amd import train as T
    parser = T.build_parser()
    args = parser.parse_args([])
    assert args.model == 'odenet'
    assert T.default_run_dir(args) == os.path.join('runs_mnist', 'odenet_residual_f64_dopri5_tol0.001')
    args = parser.parse_args(['--model', 'resnet', '--dataset', 'cifar10', '-d', 'residual', '-f', '256'])
    assert args.model == 'resnet'
    assert T.default_run_dir(args) == os.path.join('runs_cifar10', 'resnet_residual_f256')
    assert parser.parse_args(['-m', 'resnet']).model == 'resnet'
    with pytest.raises(SystemExit):
        parser.parse_args(['--model', 'vgg'])
    # refusals come before any device is touched
    with pytest.raises(SystemExit, match='deferred'):
        T.main(['--model', 'resnet', '--deferred'])
    with pytest.raises(SystemExit, match='one-shot'):
        T.main(['--model', 'resnet', '-d', 'ode'])


def test_seeds_of_the_gpu_parity_cases_have_agreeing_relu_masks():
    """tests/test_gpu_resnet.py keeps, per case, a seed at which every ReLU mask of the fp32 CPU run equals the fp64 run's (its
    docstring says how they were chosen): re-checked here for the cases of up to two blocks (the six-block ones take seconds)."""
    from tests import test_gpu_resnet as G
    for case in G.CASES:
        if case[3] <= 2:
            agree, margin = G.masks_agree(case, G.SEEDS[case])
            assert agree and margin > 1e-5, (case, margin)

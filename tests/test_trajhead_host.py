"""Host side (no GPU) of the head of a whole trajectory: `FCClassifier.forward` on [T, N, C, H, W], `ODENet.forward` and
`ResNet.forward` handing the trajectory to the head in one call, `trajectory_loss` and `trajectory_distance` on CPU tensors, and the
C ABI of the three entry points added for them (node_head_loss_slices_fwd, node_bnhead_fwd_slices, node_gn_relu_distance): exports,
the layout of the one new structure, and the refusals, every one of which returns before a launch."""
import copy
import ctypes as C
import os
import subprocess

import pytest
import torch
from torch import nn

from tests import trajhead_cases as K

NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED, NODE_ERR_ARG = -1, -2, -3, -9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('node_head_loss_slices_scratch_bytes', 'node_head_loss_slices_fwd', 'node_bnhead_slices_scratch_bytes',
         'node_bnhead_fwd_slices', 'node_gn_relu_distance')


# ---------------------------------------------------------------------------------------------------------------------
# the head on a CPU trajectory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('features', [False, True], ids=['linear', 'pool_only'])
@pytest.mark.parametrize('norm', ['group', 'batch'])
@pytest.mark.parametrize('case', K.CPU_HEAD_CASES, ids=str)
def test_classifier_takes_a_cpu_trajectory_as_the_stacked_slices(case, norm, features):
    T, n, c = case[:3]
    head = K.classifier(c, 10, norm=norm, features=features)
    x = K.trajectory(case)
    with torch.no_grad():
        want = torch.stack([head(xi) for xi in x])
        got = head(x)
    assert got.shape == (T, n, c if features else 10)
    assert torch.equal(got, want)
    if norm == 'batch':      # per-slice statistics: NOT the flattened batch
        with torch.no_grad():
            flat = head(x.reshape(T * n, *case[2:])).reshape(got.shape)
        assert not torch.equal(got, flat)


def test_classifier_trajectory_keeps_the_loop_where_the_issue_says_so():
    """`_trajectory_fusable` is False for every CPU tensor; its other refusals are decided before the device is looked at only for
    `fused_trajectory = False`, so they are checked on the predicate's parts: hooks, dropout in training mode, an edited body."""
    import neural_ode_features_amd as nof
    assert nof.FCClassifier.fused_trajectory is True
    head = K.classifier(64, 10)
    x = K.trajectory((2, 2, 64, 4, 4))
    assert not head._trajectory_fusable(x)                           # a CPU tensor

    class _Cuda:           # what the predicate reads of a tensor: a HIP fp32 trajectory that is never touched
        is_cuda, dtype, shape = True, torch.float32, (2, 2, 64, 4, 4)
    assert head._trajectory_fusable(_Cuda())
    handle = head.module[0].register_forward_hook(lambda m, i, o: None)
    assert not head._trajectory_fusable(_Cuda())
    handle.remove()
    handle = head.register_forward_pre_hook(lambda m, i: None)
    assert not head._trajectory_fusable(_Cuda())
    handle.remove()
    assert head._trajectory_fusable(_Cuda())
    dropped = nof.FCClassifier(64, 10, dropout=0.5)
    assert not dropped.train()._trajectory_fusable(_Cuda()) and dropped.eval()._trajectory_fusable(_Cuda())
    edited = K.classifier(64, 10)
    edited.module[1] = nn.Tanh()
    assert not edited._trajectory_fusable(_Cuda())
    try:
        nof.FCClassifier.fused_trajectory = False
        assert not head._trajectory_fusable(_Cuda())
    finally:
        nof.FCClassifier.fused_trajectory = True
    # dropout in training mode: one mask per slice, drawn in the loop's order
    torch.manual_seed(3)
    want = torch.stack([dropped.train()(xi) for xi in x])
    torch.manual_seed(3)
    assert torch.equal(dropped(x), want)


def _nets():
    import neural_ode_features_amd as nof
    torch.manual_seed(2)
    ode = nof.ODENet(3, n_filters=16, downsample='one-shot')
    ode.odeblock = K.Trajectory(3)
    ode.to_features_extractor()
    ode2 = nof.ODENet(3, n_filters=16, downsample='one-shot')
    ode2.odeblock = K.Trajectory(3)
    ode2.odeblock.return_last_only = False           # the accuracy sweep: the classification layer on every slice
    res = nof.ResNet(3, n_filters=16, downsample='one-shot')
    res.to_features_extractor()
    unpooled = nof.ODENet(3, n_filters=16, downsample='one-shot')
    unpooled.odeblock = K.Trajectory(3)
    unpooled.to_features_extractor(keep_pool=False)
    return {'odenet_features': (ode, (3, 2, 16)), 'odenet_logits': (ode2, (3, 2, 10)), 'resnet_features': (res, (7, 2, 16)),
            'odenet_unpooled': (unpooled, (3, 2, 16, 8, 8))}


@pytest.mark.parametrize('name', ['odenet_features', 'odenet_logits', 'resnet_features', 'odenet_unpooled'])
def test_cpu_nets_return_the_same_with_the_trajectory_call_on_and_off(name):
    import neural_ode_features_amd as nof
    net, shape = _nets()[name]
    net.eval()
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        on = net(x)
        try:
            nof.FCClassifier.fused_trajectory = False
            off = net(x)
        finally:
            nof.FCClassifier.fused_trajectory = True
    assert on.shape == shape and torch.equal(on, off)


def test_a_hooked_head_still_sees_every_slice():
    net, _ = _nets()['odenet_features']
    seen = []
    handle = net.classifier.register_forward_hook(lambda m, i, o: seen.append(tuple(i[0].shape)))
    with torch.no_grad():
        net.eval()(torch.randn(2, 3, 16, 16))
    handle.remove()
    assert seen == [(2, 16, 8, 8)] * 3


def test_resnet_taps_come_as_one_tensor_or_as_the_list():
    import neural_ode_features_amd as nof
    torch.manual_seed(0)
    trunk = nof.ResidualTrunk(16, 6)
    x = torch.randn(2, 16, 8, 8)
    with torch.no_grad():
        out, taps = trunk.forward_taps(x)
        out2, taps2 = trunk.forward_taps_stacked(x)
    assert isinstance(taps, list) and isinstance(taps2, list) and len(taps) == 6         # CPU: the modules ran
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(taps, taps2))


# ---------------------------------------------------------------------------------------------------------------------
# the public functions on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.LOSS_CASES, ids=str)
def test_trajectory_loss_on_the_cpu_against_an_fp64_loop(case):
    import neural_ode_features_amd as nof
    pooled, weight, bias, target = K.loss_inputs(case)
    logits = pooled @ weight.t() + bias
    stat = nof.trajectory_loss(logits, target)
    assert stat.shape == (case[0], 2) and stat.dtype == torch.float32
    loss, hits = K.loss_fp64(logits, target)
    assert torch.equal(stat[:, 1].double(), hits)
    # fp32 log-softmax of `classes` terms and a sum of N of them: a few ulp of the largest term each
    assert float((stat[:, 0].double() - loss).abs().max()) <= 1e-5 * max(1.0, float(loss.abs().max()))
    s64 = nof.trajectory_loss(logits.double(), target)
    assert s64.dtype == torch.float64 and float((s64[:, 0] - loss).abs().max()) <= 1e-12 * max(1.0, float(loss.abs().max()))
    with pytest.raises(ValueError):
        nof.trajectory_loss(logits[0], target)
    with pytest.raises(ValueError):
        nof.trajectory_loss(logits, target[:-1] if case[1] > 1 else torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize('case', [(3, 2, 64, 8, 8), (2, 3, 64, 7, 7)], ids=str)
def test_trajectory_distance_on_the_cpu_against_an_fp64_loop(case):
    import neural_ode_features_amd as nof
    traj0, traj1, norm, l2_64, cos_64 = K.distance_case(case)
    l2, cos = nof.trajectory_distance(traj0, traj1, norm)
    assert l2.shape == cos.shape == case[:2]
    want_l2, want_cos = K.aten_distance(traj0, traj1, norm)               # the chain `attack diff` runs
    assert torch.allclose(l2, want_l2, rtol=1e-6, atol=0) and torch.allclose(cos, want_cos, rtol=0, atol=1e-6)
    assert float(((l2.double() - l2_64) / l2_64).abs().max()) <= 1e-5 and float((cos.double() - cos_64).abs().max()) <= 1e-5
    l2, cos = nof.trajectory_distance(traj0.double(), traj1.double(), copy.deepcopy(norm).double())
    assert float(((l2 - l2_64) / l2_64).abs().max()) <= 1e-12 and float((cos - cos_64).abs().max()) <= 1e-12
    with pytest.raises(ValueError):
        nof.trajectory_distance(traj0, traj1[:-1], norm)
    with pytest.raises(ValueError):
        nof.trajectory_distance(traj0[0], traj1[0], norm)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_abi_version():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in CALLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additions only
    header = open(os.path.join(ROOT, 'include', 'node_hip.h')).read()
    for proto in ('size_t node_head_loss_slices_scratch_bytes(int slices, int n);',
                  'int node_head_loss_slices_fwd(const node_head_loss_slices* head, void* stream);',
                  'size_t node_bnhead_slices_scratch_bytes(const node_bnfunc_shape* shape, int slices);',
                  'int node_bnhead_fwd_slices(const node_bnfunc_shape* shape, int slices, const float* z, const float* gamma, const float* beta,',
                  'int node_gn_relu_distance(const node_shape* shape /* n = rows */, const float* a, const float* b, const float* gamma,'):
        assert proto in header, proto


def test_ctypes_layout_of_the_sliced_loss_matches_the_header(tmp_path):
    """The gcc `offsetof` program of tests/test_bnconvstem_host.py for the one structure added; node_head_loss keeps its layout."""
    from neural_ode_features_amd import _lib
    fields = ['slices', 'n', 'c', 'classes', 'pooled', 'weight', 'bias', 'target', 'logits', 'loss', 'stat', 'scratch']
    structs = {'node_head_loss_slices': (_lib.NodeHeadLossSlices, fields),
               'node_head_loss': (_lib.NodeHeadLoss, ['n', 'c', 'classes', 'reduction'] + fields[4:])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {']
    for name, (_, fs) in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fs:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    lines += ['  printf("abi %d\\n", NODE_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / 'abi.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, (ct, fs) in structs.items():
        assert int(got[name]) == C.sizeof(ct), name
        assert [k for k, _ in ct._fields_] == fs
        for f in fs:
            assert int(got['%s.%s' % (name, f)]) == getattr(ct, f).offset, (name, f)
    assert int(got['abi']) == 6
    assert C.sizeof(_lib.NodeHeadLossSlices) == 80


def _host_buffer():
    buf = (C.c_char * 16384)()
    return buf, (C.addressof(buf) + 255) & ~255


def test_sliced_loss_refusals_return_before_any_launch():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    buf, base = _host_buffer()
    H = _lib.NodeHeadLossSlices
    size, fwd = lib.node_head_loss_slices_scratch_bytes, lib.node_head_loss_slices_fwd
    p = [base + 256 * k for k in range(8)]         # pooled, weight, bias, target, logits, loss, stat, scratch: host memory, never read

    def head(slices=3, n=5, c=64, classes=10, hole=()):
        v = [None if k in hole else p[k] for k in range(8)]
        return C.byref(H(slices, n, c, classes, *v))
    assert size(3, 5) == (4 + 3 * 2 * 2) * 4 and size(21, 7) == (24 + 21 * 2 * 2) * 4 and size(1, 1) == (4 + 2) * 4
    for slices, n in ((0, 5), (-1, 5), (3, 0), (65536, 5)):
        assert size(slices, n) == 0
    assert fwd(None, None) == NODE_ERR_NULL
    assert fwd(head(slices=0), None) == NODE_ERR_SHAPE and b'slices' in lib.node_last_error()
    assert fwd(head(n=0), None) == NODE_ERR_SHAPE
    assert fwd(head(classes=1025), None) == NODE_ERR_UNSUPPORTED and b'1024 classes' in lib.node_last_error()
    assert fwd(head(slices=65536), None) == NODE_ERR_UNSUPPORTED and b'65535 slices' in lib.node_last_error()
    assert fwd(head(hole=(4,)), None) == NODE_ERR_NULL and b'logits' in lib.node_last_error()
    assert fwd(head(hole=(1,)), None) == NODE_ERR_NULL                                      # pooled without weight
    assert fwd(head(hole=(0, 3)), None) == NODE_ERR_ARG and b'nothing to do' in lib.node_last_error()
    assert fwd(head(hole=(5, 6)), None) == NODE_ERR_NULL                                    # a target, and nowhere to write
    assert fwd(head(hole=(7,)), None) == NODE_ERR_NULL and b'scratch' in lib.node_last_error()
    assert fwd(head(c=100000, classes=1024), None) == NODE_ERR_UNSUPPORTED and b'in_features' in lib.node_last_error()
    del buf


def test_sliced_batch_norm_head_refuses_what_the_head_refuses():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    buf, base = _host_buffer()
    S = _lib.NodeBnfuncShape
    size, fwd = lib.node_bnhead_slices_scratch_bytes, lib.node_bnhead_fwd_slices
    z, g, b, pooled, stats, scratch = (base + 256 * k for k in range(6))
    good = S(2, 64, 8, 8, 1e-5)
    one = lib.node_bnhead_scratch_bytes(C.byref(good))
    assert one > 0 and size(C.byref(good), 3) == 3 * one and size(C.byref(good), 1) == one
    for bad, word, code in ((S(2, 96, 8, 8, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED), (S(2, 32, 8, 8, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED),
                            (S(2, 8192, 8, 8, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED), (S(0, 64, 8, 8, 1e-5), 'shape', NODE_ERR_SHAPE),
                            (S(40000, 256, 16, 16, 1e-5), '2^31', NODE_ERR_UNSUPPORTED)):
        assert lib.node_bnhead_scratch_bytes(C.byref(bad)) == 0            # what node_bnhead_fwd refuses ...
        assert size(C.byref(bad), 3) == 0                                  # ... the sliced entry refuses
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert fwd(C.byref(bad), 3, z, g, b, pooled, stats, scratch, None) == code
    for slices in (0, -2, 65536):
        assert size(C.byref(good), slices) == 0 and b'slices' in lib.node_last_error()
        assert fwd(C.byref(good), slices, z, g, b, pooled, stats, scratch, None) == NODE_ERR_UNSUPPORTED
    assert size(None, 3) == 0 and fwd(None, 3, z, g, b, pooled, stats, scratch, None) == NODE_ERR_NULL
    s = C.byref(good)
    for hole in range(6):
        args = [z, g, b, pooled, stats, scratch]
        args[hole] = None
        assert fwd(s, 3, *args, None) == NODE_ERR_NULL, hole
    assert fwd(s, 3, z + 2, g, b, pooled, stats, scratch, None) == NODE_ERR_ARG
    assert fwd(s, 3, z, g, b, pooled, stats, scratch + 4, None) == NODE_ERR_ARG and b'8-byte' in lib.node_last_error()
    del buf


def test_distance_refusals_return_before_any_launch():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    buf, base = _host_buffer()
    S = _lib.NodeShape
    fn = lib.node_gn_relu_distance
    a, b, g, bt, out = (base + 256 * k for k in range(5))
    good = C.byref(S(6, 64, 8, 8, 32, 1e-5))
    assert fn(None, a, b, g, bt, out, None) == NODE_ERR_NULL
    assert fn(C.byref(S(0, 64, 8, 8, 32, 1e-5)), a, b, g, bt, out, None) == NODE_ERR_SHAPE
    assert fn(C.byref(S(6, 64, 8, 8, 24, 1e-5)), a, b, g, bt, out, None) == NODE_ERR_SHAPE and b'divide' in lib.node_last_error()
    assert fn(C.byref(S(6, 384, 8, 8, 32, 1e-5)), a, b, g, bt, out, None) == NODE_ERR_UNSUPPORTED and b'straddle' in lib.node_last_error()
    assert fn(C.byref(S(6, 8192, 8, 8, 32, 1e-5)), a, b, g, bt, out, None) == NODE_ERR_UNSUPPORTED
    for hole in range(5):
        args = [a, b, g, bt, out]
        args[hole] = None
        assert fn(good, *args, None) == NODE_ERR_NULL, hole
    assert fn(good, a + 4, b, g, bt, out, None) == NODE_ERR_ARG and b'16-byte' in lib.node_last_error()
    assert fn(good, a, b + 8, g, bt, out, None) == NODE_ERR_ARG
    del buf

"""Host side (no GPU) of the `norm='batch'` dynamics node (bnfunc.py, csrc/bnfunc_api.hip): the command line, the argument
checks of node_bnfunc_*, the ctypes layouts, the CPU path of `ODEfunc(C, norm='batch')`, the seeds of
tests/test_gpu_bnfunc.py, and the conditions of its multi-row cases: their launch regimes through node_bnfunc_describe, the
signs of their special parameter sets, the margins of their ordinary seeds."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from tests import bnfunc_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_ERR_NULL, NODE_ERR_WORKSPACE, NODE_ERR_ARG = -1, -4, -9


def test_norm_batch_parses_and_group_run_directories_keep_their_names():
    from neural_ode_features_amd import train as T
    p = T.build_parser()
    assert p.parse_args(['--norm', 'batch']).norm == 'batch' and p.parse_args(['-n', 'batch']).norm == 'batch'
    assert p.parse_args([]).norm == 'group'
    with pytest.raises(SystemExit):
        p.parse_args(['--norm', 'layer'])
    assert T.default_run_dir(p.parse_args([])) == os.path.join('runs_mnist', 'odenet_residual_f64_dopri5_tol0.001')
    assert T.default_run_dir(p.parse_args(['-a', '--dataset', 'cifar10', '-f', '256'])) == \
        os.path.join('runs_cifar10', 'odenet_residual_f256_dopri5_tol0.001_adjoint')
    assert T.default_run_dir(p.parse_args(['--model', 'resnet'])) == os.path.join('runs_mnist', 'resnet_residual_f64')
    assert T.default_run_dir(p.parse_args(['-n', 'batch', '-a'])) == os.path.join('runs_mnist', 'odenet_residual_f64_dopri5_tol0.001_adjoint_batch')
    with pytest.raises(SystemExit, match='generic solver'):
        T.main(['--norm', 'batch', '--deferred', '-a'])


def test_workspace_sizes_and_refusals():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeBnfuncShape
    size = lambda s, keep: lib.node_bnfunc_workspace_bytes(C.byref(s), keep)
    for shape in ((128, 256, 8, 8), (32, 64, 7, 7)):
        s = S(*shape, 1e-5)
        assert size(s, 0) > 0 and size(s, 1) > size(s, 0), shape
    assert size(S(2, 192, 8, 8, 1e-5), 1) > 0                # BatchNorm has no groups: any multiple of 64
    for bad, word in ((S(2, 16, 8, 8, 1e-5), 'multiple of 64'), (S(2, 96, 8, 8, 1e-5), 'multiple of 64'), (S(2, 64, 2, 8, 1e-5), 'h, w >= 3'),
                      (S(2, 64, 8, 2, 1e-5), 'h, w >= 3'), (S(8192, 4096, 8, 8, 1e-5), '2^31'), (S(0, 64, 8, 8, 1e-5), 'shape'),
                      (S(2, 8192, 8, 8, 1e-5), 'multiple of 64')):
        for keep in (0, 1):
            assert size(bad, keep) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_bnfunc_fwd(C.byref(bad), None, None, None, None, 1, None, 0, None) == \
            (_lib.NODE_ERR_UNSUPPORTED if word != 'shape' else -2)
    assert lib.node_bnfunc_workspace_bytes(None, 1) == 0


def test_null_misaligned_and_short_workspace_arguments_are_rejected_before_any_launch():
    """Every call below returns before its first launch (this test runs without a GPU); the pointers are host memory that is
    never read."""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeBnfuncShape(2, 64, 8, 8, 1e-5)
    nbytes = lib.node_bnfunc_workspace_bytes(C.byref(shape), 1)
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 255) & ~255
    P = _lib.NodeBnfuncParams
    good = P(*[base + 256 * i for i in range(10)])
    holed = P(*[base + 256 * i if i != 6 else None for i in range(10)])
    odd = P(*[base + 256 * i + (4 if i == 2 else 0) for i in range(10)])
    t, x, out, ws = base + 2560, base + 2816, base + 3072, base + 3328
    fwd, bwd = lib.node_bnfunc_fwd, lib.node_bnfunc_bwd
    s = C.byref(shape)
    assert fwd(None, C.byref(good), t, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, None, t, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, C.byref(holed), t, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, C.byref(odd), t, x, out, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, C.byref(good), None, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, C.byref(good), t, None, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, C.byref(good), t, x, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, C.byref(good), t, x + 4, out, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, C.byref(good), t, x, out, 1, None, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, C.byref(good), t, x, out, 1, ws + 16, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, C.byref(good), t, x, out, 1, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    assert 'too small' in lib.node_last_error().decode()
    assert fwd(s, C.byref(good), t, x, out, 0, ws, lib.node_bnfunc_workspace_bytes(s, 0) - 1, None) == NODE_ERR_WORKSPACE
    dx, dt = out, t + 4
    assert bwd(None, C.byref(good), t, x, C.byref(good), dx, dt, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, None, t, x, C.byref(good), dx, dt, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, C.byref(good), None, x, C.byref(good), dx, dt, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, C.byref(good), t, None, C.byref(good), dx, dt, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, C.byref(good), t, x, C.byref(holed), dx, dt, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, C.byref(good), t, x, C.byref(odd), dx, dt, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, C.byref(good), t, x, C.byref(good), dx + 8, dt, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, C.byref(good), t, x, C.byref(good), dx, dt + 2, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, C.byref(good), t, x, C.byref(good), dx, dt, None, nbytes, None) == NODE_ERR_NULL
    # grads, d_x and d_t are optional (NULL: not wanted): the next check, the workspace's size, is reached
    assert bwd(s, C.byref(good), t, x, None, None, None, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    assert bwd(s, C.byref(good), t, x, C.byref(good), dx, dt, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE


def test_ctypes_layouts_match_the_header(tmp_path):
    """tests/test_convstem_host.py::test_ctypes_layouts_of_the_new_structs_match_the_header for the structs of this addition."""
    from neural_ode_features_amd import _lib
    structs = {
        'node_bnfunc_shape': (_lib.NodeBnfuncShape, ['n', 'channels', 'h', 'w', 'eps']),
        'node_bnfunc_params': (_lib.NodeBnfuncParams, list(_lib.BNFUNC_PARAM_FIELDS)),
        'node_bnfunc_grads': (_lib.NodeBnfuncParams, list(_lib.BNFUNC_PARAM_FIELDS)),
        'node_bnfunc_info': (_lib.NodeBnfuncInfo, ['rows', 'chunk_rows', 'nchunk', 'last_chunk_rows', 'column_tiles', 'wgrad_nsplit',
                                                   'wgrad_rows_per_split']),
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
    assert [k for k, _ in _lib.NodeBnfuncInfo._fields_] == structs['node_bnfunc_info'][1]
    assert all(ct is C.c_int32 for _, ct in _lib.NodeBnfuncInfo._fields_)
    for name in ('node_bnfunc_workspace_bytes', 'node_bnfunc_fwd', 'node_bnfunc_bwd', 'node_bnfunc_describe'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.load().node_abi_version() == 6 == _lib.NODE_ABI_VERSION
    # the ten tensors are ODEfunc's own, in named_parameters() order
    import neural_ode_features_amd as nof
    names = [k for k, _ in nof.ODEfunc(64, norm='batch').named_parameters()]
    assert [n.replace('._layer', '').replace('.weight', '_w').replace('.bias', '_b') for n in names] == list(_lib.BNFUNC_PARAM_FIELDS)


def test_cpu_tensors_run_the_module_operations_and_recognised_still_raises():
    import torch.nn.functional as F
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import bnfunc, integrate
    func, _ = B.func_pair(64, seed=3)
    assert nof.ODEfunc.fused_batch is True
    x = torch.randn(2, 64, 8, 8).requires_grad_(True)
    t = torch.tensor(0.37)
    assert bnfunc.plan(func, t, x) is None
    out = func(t, x)
    assert type(out.grad_fn).__name__ != '_BatchOdeFnBackward' and func.nfe == 1
    h = F.relu(func.norm1(x))
    h = F.relu(func.norm2(func.conv1(t, h)))
    assert torch.equal(out, func.norm3(func.conv2(t, h)))
    with pytest.raises(NotImplementedError):
        integrate.Recognised(func)
    # what the node is offered: the reference's BatchNorm2d(track_running_stats=False) alone
    assert bnfunc._norms_and_convs(func) is not None
    assert bnfunc._norms_and_convs(nof.ODEfunc(64, norm='group')) is None
    tracked = nof.ODEfunc(64, norm='batch')
    tracked.norm2 = torch.nn.BatchNorm2d(64)
    assert bnfunc._norms_and_convs(tracked) is None


@pytest.mark.parametrize('case', B.CASES, ids=lambda c: 'n%d_c%d_%dx%d' % c)
def test_seeds_of_the_gpu_cases_keep_every_relu_mask(case):
    """The seeds tests/test_gpu_bnfunc.py runs its ordinary-parameter cases with: every ReLU mask of the fp32 CPU run agrees with the
    fp64 run's (bnfunc_cases.py has the recipe)."""
    agree, margin = B.masks_agree(case, B.SEEDS[case])
    assert agree and margin > 0


def _id(c):
    return 'n%d_c%d_%dx%d' % c


def test_plan_query_is_consistent_and_refuses_what_the_node_refuses():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    info = _lib.NodeBnfuncInfo()
    assert lib.node_bnfunc_describe(None, C.byref(info)) == NODE_ERR_NULL
    assert lib.node_bnfunc_describe(C.byref(_lib.NodeBnfuncShape(2, 64, 8, 8, 1e-5)), None) == NODE_ERR_NULL
    assert lib.node_bnfunc_describe(C.byref(_lib.NodeBnfuncShape(2, 96, 8, 8, 1e-5)), C.byref(info)) == _lib.NODE_ERR_UNSUPPORTED
    assert info.rows == 0 and 'multiple of 64' in lib.node_last_error().decode()
    with pytest.raises(_lib.NodeHipError):
        _lib.describe_bnfunc(2, 64, 2, 8)
    for case in list(B.CASES) + list(B.MULTI_CASES) + [(128, 256, 8, 8)]:
        d = _lib.describe_bnfunc(*case)
        assert d['rows'] == case[0] * case[2] * case[3] and d['column_tiles'] * 64 == case[1]
        assert d['chunk_rows'] % 32 == 0 and (d['nchunk'] - 1) * d['chunk_rows'] + d['last_chunk_rows'] == d['rows']
        assert 0 < d['last_chunk_rows'] <= d['chunk_rows']
        assert (d['wgrad_nsplit'] - 1) * d['wgrad_rows_per_split'] < d['rows'] <= d['wgrad_nsplit'] * d['wgrad_rows_per_split']
    assert _lib.describe_bnfunc(128, 256, 8, 8)['chunk_rows'] > 64         # the CIFAR training step: four trips of the row loops


@pytest.mark.parametrize('case', B.CASES, ids=_id)
def test_the_first_cases_all_run_one_trip_of_the_row_loops(case):
    """Why B.MULTI_CASES exists: every case of B.CASES has chunks of 32 rows, so no thread of a BatchNorm pass takes a second
    trip round `for (r = r0 + rr; r < r1; r += 32)`."""
    from neural_ode_features_amd import _lib
    assert _lib.describe_bnfunc(*case)['chunk_rows'] == 32


@pytest.mark.parametrize('case', B.MULTI_CASES, ids=_id)
def test_new_cases_are_in_the_regimes_they_are_there_for(case):
    from neural_ode_features_amd import _lib
    d = _lib.describe_bnfunc(*case)
    assert B.MULTI_CASES[case], case
    for regime in B.MULTI_CASES[case]:
        assert B.REGIMES[regime](d), (case, regime, d)


def test_new_cases_cover_every_regime_between_them():
    named = {r for regimes in B.MULTI_CASES.values() for r in regimes}
    assert named == set(B.REGIMES), named ^ set(B.REGIMES)
    # what the lane model says of the split counts the suite runs: 1, 2, 4 remainder only; 8, 64 loop only
    for ns in (1, 2, 4):
        assert B.reduce_lanes(ns)[0] == set()
    for ns in (8, 64):
        assert B.reduce_lanes(ns) == ({0, 1, 2, 3}, set())
    assert B.reduce_lanes(5) == ({0}, {1, 2, 3}) and B.reduce_lanes(52) == ({0, 1, 2, 3}, {0, 1, 2, 3})


@pytest.mark.parametrize('mode', ['kinkfree', 'split'])
@pytest.mark.parametrize('case', B.MULTI_CASES, ids=_id)
def test_special_parameter_sets_keep_every_preactivation_clear_of_zero(case, mode):
    """A condition of the GPU tests, not a measurement: in fp64 every channel of norm1's and norm2's output has one sign over all rows
    and no |pre-activation| is under 0.1; 'split' masks exactly half the channels, 'kinkfree' none."""
    constant, on, margin = B.sign_condition(case, B.KINK_FREE_SEED, mode)
    assert constant and margin >= 0.1, (constant, margin)
    assert on == ([0.5, 0.5] if mode == 'split' else [1.0, 1.0]), on


@pytest.mark.parametrize('case', B.MULTI_CASES, ids=_id)
def test_ordinary_seeds_of_the_new_cases_are_admissible(case):
    """The kept seed alone is re-checked (bnfunc_cases.py has the recipe and the search): every ReLU mask of the fp32 CPU run agrees
    with the fp64 run's, and margin / error is at least that of the closest case the suite ran before, computed here."""
    if case not in B.MULTI_SEEDS:
        return                   # no admissible seed in 0..199: the case runs kink-free and split only
    need = B.margin_ratio(*B.RATIO_YARDSTICK)[2]
    agree, margin, ratio = B.margin_ratio(case, B.MULTI_SEEDS[case])
    print('%s seed %d: margin %.2e, margin / error %.2f (needed %.2f)' % (case, B.MULTI_SEEDS[case], margin, ratio, need))
    assert agree and margin > 0 and ratio >= need, (agree, margin, ratio, need)

"""Host side (no GPU) of the batch-norm solve (bnsolve.py, csrc/bnsolve_api.hip): the ctypes layout of node_bnsolve_opts, the
workspace query and its refusals, the argument checks of node_bnsolve_fwd / node_bnsolve_adjoint (every call here returns before
its first launch), `bnsolve.plan` on tensors that claim a device, the switch `build_model` sets, and the command line."""
import ctypes as C
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED, NODE_ERR_WORKSPACE, NODE_ERR_ARG = -1, -2, -3, -4, -9
DOPRI5, RK4 = 0, 1


def test_ctypes_layout_of_the_options_matches_the_header(tmp_path):
    from neural_ode_features_amd import _lib
    fields = ['max_num_steps', 'steps_hint', 'grad_last_only']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "node_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(node_bnsolve_opts));']
    lines += ['  printf("%s %%zu\\n", offsetof(node_bnsolve_opts, %s));' % (f, f) for f in fields]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'abi.c', tmp_path / 'abi'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['size']) == C.sizeof(_lib.NodeBnsolveOpts)
    assert [f for f, _ in _lib.NodeBnsolveOpts._fields_] == fields
    for f in fields:
        assert int(got[f]) == getattr(_lib.NodeBnsolveOpts, f).offset, f
    for name in ('node_bnsolve_workspace_bytes', 'node_bnsolve_fwd', 'node_bnsolve_adjoint'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.load().node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additive


def test_launch_regimes_of_the_solve_shapes():
    """A solve runs the plan node_bnfunc_describe reports (bnsolve_api.hip takes make_bn_plan's): every shape of SHAPES and
    SPLITK_SHAPE has chunks of 32 rows -- one trip of the BatchNorm passes' row loops -- and MULTIROW_SHAPE is there for the second
    trip and a last chunk shorter than the 32 row slots."""
    from neural_ode_features_amd import _lib
    from tests import bnsolve_cases as S
    for shape in S.SHAPES + [S.SPLITK_SHAPE]:
        assert _lib.describe_bnfunc(*shape)['chunk_rows'] == 32, shape
    assert _lib.describe_bnfunc(*S.SPLITK_SHAPE)['wgrad_nsplit'] > 8
    d = _lib.describe_bnfunc(*S.MULTIROW_SHAPE)
    assert d['chunk_rows'] > 32 and 0 < d['last_chunk_rows'] < 32 and d['wgrad_nsplit'] > 8, d


def test_workspace_query_sizes_and_refusals():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeBnfuncShape
    size = lambda s, method=DOPRI5, adjoint=0, n_t=2: lib.node_bnsolve_workspace_bytes(C.byref(s), method, adjoint, n_t)
    for shape in ((128, 256, 8, 8), (4, 64, 6, 6), (1, 64, 3, 3), (2, 192, 7, 7)):
        s = S(*shape, 1e-5)
        one = lib.node_bnfunc_workspace_bytes(C.byref(s), 1)
        assert size(s, adjoint=1) > size(s) > lib.node_bnfunc_workspace_bytes(C.byref(s), 0), shape
        assert size(s, adjoint=1) > one
        assert size(s, RK4, 1, 4) > size(s, RK4, 1, 2)                      # the NHWC slices grow with n_t
        # the adjoint holds ten flat buffers (y, y1, a stage state, seven stage derivatives) of each of y, adj_y and adj_params
        n, c, h, w = shape
        flat = 4 * 10 * (2 * n * c * h * w + 2 * c * (c + 1) * 9 + 8 * c)
        assert size(s, adjoint=1) >= one + flat
    # the shapes check_bn_shape refuses, with its words
    for bad, word in ((S(2, 16, 8, 8, 1e-5), 'multiple of 64'), (S(2, 96, 8, 8, 1e-5), 'multiple of 64'), (S(2, 64, 2, 8, 1e-5), 'h, w >= 3'),
                      (S(2, 64, 8, 2, 1e-5), 'h, w >= 3'), (S(8192, 4096, 8, 8, 1e-5), '2^31'), (S(0, 64, 8, 8, 1e-5), 'shape'),
                      (S(2, 8192, 8, 8, 1e-5), 'multiple of 64')):
        for adjoint in (0, 1):
            assert size(bad, adjoint=adjoint) == 0, bad
            assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        code = NODE_ERR_SHAPE if word == 'shape' else NODE_ERR_UNSUPPORTED
        assert lib.node_bnsolve_fwd(C.byref(bad), None, None, None, 2, 1e-3, 1e-3, DOPRI5, None, None, None, None, 0, None) == code
        assert lib.node_bnsolve_adjoint(C.byref(bad), None, None, None, None, 2, 1e-3, 1e-3, DOPRI5, None, None, None, None, None, 0, None) == code
    good = S(2, 64, 8, 8, 1e-5)
    assert lib.node_bnsolve_workspace_bytes(None, DOPRI5, 1, 2) == 0
    # the slices of one call together stay under 2^31 elements (the boundary's layout launches take them at once); n_t <= 1024
    big = S(4096, 256, 8, 8, 1e-5)                     # 2^26 elements a slice
    assert size(big, n_t=31) > 0 and size(big, n_t=32) == 0 and '2^31' in lib.node_last_error().decode()
    assert lib.node_bnsolve_fwd(C.byref(big), C.byref(_lib.NodeBnfuncParams(*[256 * (i + 1) for i in range(10)])), None,
                                (C.c_float * 32)(*range(32)), 32, 1e-3, 1e-3, DOPRI5, None, None, None, None, 0, None) == NODE_ERR_UNSUPPORTED
    assert size(good, n_t=1024) > 0 and size(good, n_t=1025) == 0 and 'n_t' in lib.node_last_error().decode()
    assert size(good, method=2) == 0 and 'method' in lib.node_last_error().decode()
    assert size(good, n_t=1) == 0 and 'n_t' in lib.node_last_error().decode()


def _args():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeBnfuncShape(2, 64, 8, 8, 1e-5)
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 255) & ~255
    P = _lib.NodeBnfuncParams
    good = P(*[base + 256 * i for i in range(10)])
    holed = P(*[base + 256 * i if i != 6 else None for i in range(10)])
    odd = P(*[base + 256 * i + (4 if i == 2 else 0) for i in range(10)])
    return lib, shape, buf, base, good, holed, odd


def test_forward_arguments_are_rejected_before_any_launch():
    """The pointers are host memory that is never read: every call returns at a check."""
    from neural_ode_features_amd import _lib
    lib, shape, buf, base, good, holed, odd = _args()
    s = C.byref(shape)
    nbytes = lib.node_bnsolve_workspace_bytes(s, DOPRI5, 0, 3)
    y0, out, ws = base + 2560, base + 2816, base + 3328
    t = (C.c_float * 3)(0.0, 0.5, 1.0)
    stats = _lib.NodeStats()
    opts = _lib.NodeBnsolveOpts(0, 0, 0)

    def fwd(shape=s, prm=C.byref(good), y0=y0, t=t, n_t=3, method=DOPRI5, out=out, ws=ws, nbytes=nbytes):
        return lib.node_bnsolve_fwd(shape, prm, y0, t, n_t, 1e-3, 1e-3, method, C.byref(opts), out, C.byref(stats), ws, nbytes, None)
    assert fwd(shape=None) == NODE_ERR_NULL
    assert fwd(prm=None) == NODE_ERR_NULL
    assert fwd(prm=C.byref(holed)) == NODE_ERR_NULL
    assert fwd(prm=C.byref(odd)) == NODE_ERR_ARG
    assert fwd(y0=None) == NODE_ERR_NULL
    assert fwd(y0=y0 + 4) == NODE_ERR_ARG
    assert fwd(out=None) == NODE_ERR_NULL
    assert fwd(out=out + 8) == NODE_ERR_ARG
    assert fwd(t=None) == NODE_ERR_NULL
    assert fwd(method=2) == NODE_ERR_ARG
    assert fwd(ws=None) == NODE_ERR_NULL
    assert fwd(ws=ws + 16) == NODE_ERR_ARG
    assert fwd(nbytes=nbytes - 1) == NODE_ERR_WORKSPACE and 'too small' in lib.node_last_error().decode()
    # time grids: at least two points, strictly monotonic either way
    assert fwd(n_t=1) == NODE_ERR_ARG and fwd(n_t=0) == NODE_ERR_ARG
    for bad in ((0.0, 0.5, 0.5), (0.0, 0.5, 0.2), (1.0, 0.5, 0.7), (0.0, 0.0, 1.0), (0.0, float('nan'), 1.0)):
        assert fwd(t=(C.c_float * 3)(*bad)) == NODE_ERR_ARG, bad
        assert 'strictly' in lib.node_last_error().decode()
    # a decreasing grid is a grid: the next check (the workspace's size) is reached
    assert fwd(t=(C.c_float * 3)(1.0, 0.4, 0.0), nbytes=nbytes - 1) == NODE_ERR_WORKSPACE
    assert fwd(method=RK4, nbytes=lib.node_bnsolve_workspace_bytes(s, RK4, 0, 3) - 1) == NODE_ERR_WORKSPACE


def test_adjoint_arguments_are_rejected_before_any_launch():
    from neural_ode_features_amd import _lib
    lib, shape, buf, base, good, holed, odd = _args()
    s = C.byref(shape)
    nbytes = lib.node_bnsolve_workspace_bytes(s, DOPRI5, 1, 3)
    traj, gout, gy0, ws = base + 2560, base + 2816, base + 3072, base + 3328
    t = (C.c_float * 3)(0.0, 0.5, 1.0)
    stats = _lib.NodeStats()
    opts = _lib.NodeBnsolveOpts(0, 0, 1)

    def adj(shape=s, prm=C.byref(good), traj=traj, gout=gout, t=t, n_t=3, method=DOPRI5, gy0=gy0, grads=C.byref(good), ws=ws, nbytes=nbytes):
        return lib.node_bnsolve_adjoint(shape, prm, traj, gout, t, n_t, 1e-3, 1e-3, method, C.byref(opts), gy0, grads, C.byref(stats),
                                        ws, nbytes, None)
    assert adj(shape=None) == NODE_ERR_NULL
    assert adj(prm=None) == NODE_ERR_NULL
    assert adj(prm=C.byref(holed)) == NODE_ERR_NULL
    assert adj(prm=C.byref(odd)) == NODE_ERR_ARG
    assert adj(grads=C.byref(holed)) == NODE_ERR_NULL
    assert adj(grads=C.byref(odd)) == NODE_ERR_ARG
    assert adj(traj=None) == NODE_ERR_NULL
    assert adj(traj=traj + 4) == NODE_ERR_ARG
    assert adj(gout=None) == NODE_ERR_NULL
    assert adj(gout=gout + 4) == NODE_ERR_ARG
    assert adj(gy0=None) == NODE_ERR_NULL
    assert adj(gy0=gy0 + 8) == NODE_ERR_ARG
    assert adj(t=None) == NODE_ERR_NULL
    assert adj(n_t=1) == NODE_ERR_ARG
    assert adj(t=(C.c_float * 3)(0.0, 0.7, 0.3)) == NODE_ERR_ARG
    assert adj(method=-1) == NODE_ERR_ARG
    assert adj(ws=None) == NODE_ERR_NULL
    assert adj(ws=ws + 64) == NODE_ERR_ARG
    assert adj(nbytes=nbytes - 1) == NODE_ERR_WORKSPACE
    # the parameter gradients are optional (NULL: not wanted): the next check is reached
    assert adj(grads=None, nbytes=nbytes - 1) == NODE_ERR_WORKSPACE


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be a CUDA tensor (tests/test_imgconv_host.py): the device question of `plan` without a GPU."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def _on_fake_device(func):
    for m in func.modules():
        for name in list(m._parameters):
            t = m._parameters.pop(name)
            setattr(m, name, None if t is None else _FakeCuda(t.detach()))
    return func


def test_plan_takes_the_switch_the_options_and_the_function_it_knows():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import bnsolve
    assert nof.ODEfunc.batch_solve is False and nof.ODEfunc.fused_batch is True
    y = _FakeCuda(torch.zeros(4, 64, 6, 6))

    def func(C=64, norm='batch', switch=True):
        f = _on_fake_device(nof.ODEfunc(C, norm=norm))
        f.batch_solve = switch
        return f
    taken = bnsolve.plan(func(), y, DOPRI5, None)
    assert taken is not None and taken[0] == 1e-5 and len(taken[1]) == 10 and taken[2] == 0
    assert bnsolve.plan(func(), y, RK4, {'max_num_steps': 7})[2] == 7
    # more time points than one call takes: the generic solver (which takes up to 4096 targets)
    assert bnsolve.plan(func(), y, DOPRI5, None, 1024) is not None and bnsolve.plan(func(), y, DOPRI5, None, 1025) is None
    assert bnsolve.plan(func(192), _FakeCuda(torch.zeros(2, 192, 7, 7)), DOPRI5, {}) is not None
    # the switch: off by default, and the node's own switch counts too
    assert bnsolve.plan(func(switch=False), y, DOPRI5, None) is None
    try:
        nof.ODEfunc.fused_batch = False
        assert bnsolve.plan(func(), y, DOPRI5, None) is None
    finally:
        nof.ODEfunc.fused_batch = True
    # options: nothing but max_num_steps
    for opts in ({'record_dt': 8}, {'max_num_steps': 5, 'forced_dts': [0.1]}, {'global_norm': True}):
        assert bnsolve.plan(func(), y, DOPRI5, opts) is None, opts
    # the state: on a device, fp32, four-dimensional, of a shape the kernels take
    assert bnsolve.plan(func(), torch.zeros(4, 64, 6, 6), DOPRI5, None) is None
    assert bnsolve.plan(func(), _FakeCuda(torch.zeros(4, 64, 6, 6).double()), DOPRI5, None) is None
    assert bnsolve.plan(func(), _FakeCuda(torch.zeros(4, 64, 36)), DOPRI5, None) is None
    assert bnsolve.plan(func(), _FakeCuda(torch.zeros(4, 64, 2, 6)), DOPRI5, None) is None
    assert bnsolve.plan(func(), _FakeCuda(torch.zeros(4, 128, 6, 6)), DOPRI5, None) is None          # not the function's width
    for C in (16, 96):
        assert bnsolve.plan(func(C), _FakeCuda(torch.zeros(2, C, 6, 6)), DOPRI5, None) is None
    # parameters on the CPU
    plain = nof.ODEfunc(64, norm='batch')
    plain.batch_solve = True
    assert bnsolve.plan(plain, y, DOPRI5, None) is None
    # the function: group norm, hooks, tracked statistics, a foreign module
    assert bnsolve.plan(func(norm='group'), y, DOPRI5, None) is None
    hooked = func()
    hooked.norm2.register_forward_hook(lambda m, i, o: None)
    assert bnsolve.plan(hooked, y, DOPRI5, None) is None
    hooked = func()
    hooked.register_forward_pre_hook(lambda m, i: None)
    assert bnsolve.plan(hooked, y, DOPRI5, None) is None
    tracked = func()
    tracked.norm2 = torch.nn.BatchNorm2d(64)
    assert bnsolve.plan(tracked, y, DOPRI5, None) is None
    foreign = torch.nn.Linear(4, 4)
    foreign.batch_solve = foreign.fused_batch = True
    assert bnsolve.plan(foreign, y, DOPRI5, None) is None


def test_build_model_sets_the_switch_for_batch_norm_models_only():
    import neural_ode_features_amd as nof
    for downsample in ('residual', 'ode'):
        m = nof.build_model({'norm': 'batch', 'filters': 64, 'downsample': downsample, 'adjoint': True}, 1, 10)
        funcs = [f for f in m.modules() if isinstance(f, nof.ODEfunc)]
        assert funcs and all(f.batch_solve is True for f in funcs)
    m = nof.build_model({'norm': 'group', 'filters': 64}, 1, 10)
    funcs = [f for f in m.modules() if isinstance(f, nof.ODEfunc)]
    assert funcs and not any(f.batch_solve for f in funcs)
    assert not [f for f in nof.build_model({'model': 'resnet', 'norm': 'batch', 'filters': 64}, 1, 10).modules() if isinstance(f, nof.ODEfunc)]
    assert nof.ODEfunc.batch_solve is False and nof.ODEfunc(64, norm='batch').batch_solve is False
    assert nof.ODEBlock(64, norm='batch').odefunc.batch_solve is False


def test_command_line_is_unchanged():
    from neural_ode_features_amd import train as T
    p = T.build_parser()
    assert p.parse_args(['--norm', 'batch', '-a']).norm == 'batch' and p.parse_args([]).norm == 'group'
    assert not any('batch_solve' in a.dest or 'batch-solve' in ' '.join(a.option_strings) for a in p._actions)
    # the solve still reads its controller back once: deferred completion stays refused, with its present message
    with pytest.raises(SystemExit, match='generic solver'):
        T.main(['--norm', 'batch', '--deferred', '-a'])

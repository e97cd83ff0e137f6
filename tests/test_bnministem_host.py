"""Host side (no GPU) of the `norm='batch'` minimal stem (ministem.py `_BnMiniStemFn`, csrc/bnministem_api.hip): the ABI and the
layouts of its structures, the launch plans of the cases tests/test_gpu_bnministem.py runs (through the describe call), the argument
checks of the C ABI -- every one of which returns before a launch --, what the Python layer recognises and refuses, the CPU path,
and the seeds."""
import ctypes as C
import os
import subprocess

import pytest
import torch
from torch import nn

from tests import bnfunc_cases as B
from tests import bnministem_cases as K

NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED, NODE_ERR_WORKSPACE, NODE_ERR_ARG = -1, -2, -3, -4, -9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('node_bnministem_workspace_bytes', 'node_bnministem_describe', 'node_bnministem_fwd', 'node_bnministem_bwd')
TRIP, MAX_CHUNKS = 32, 128


ENV = 'NODE_TUNE_BNMINI_MAXCHUNK'


def chunk_rows(rows, cap=MAX_CHUNKS):
    """bnmini_chunk_rows of csrc/kernels_bnministem.hip, restated: at most `cap` chunks, whole 32-row trips."""
    cr = -(-rows // cap)
    return max(TRIP, -(-cr // TRIP) * TRIP)


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)


def _id(case):
    return '_'.join('%dx%d' % v if isinstance(v, tuple) else str(v) for v in case)


def test_exports_and_abi_version():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in CALLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additions only
    header = open(os.path.join(ROOT, 'include', 'node_hip.h')).read()
    for proto in ('size_t node_bnministem_workspace_bytes(const node_ministem_shape* shape, int keep_for_backward);',
                  'int node_bnministem_describe(const node_ministem_shape* shape, node_bnministem_info out[2]);'):
        assert proto in header


def test_ctypes_layouts_match_the_header(tmp_path):
    """The gcc `offsetof` program of tests/test_ministem_host.py for the structures these calls take; the version stays 6."""
    from neural_ode_features_amd import _lib
    structs = {
        'node_ministem_shape': (_lib.NodeMiniStemShape, ['n', 'in_ch', 'h', 'w', 'filters', 'eps']),
        'node_ministem_params': (_lib.NodeMiniStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
        'node_ministem_grads': (_lib.NodeMiniStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
        'node_bnministem_info': (_lib.NodeBnMiniStemInfo, ['rows', 'chunk_rows', 'nchunk', 'last_chunk_rows', 'trip_rows', 'wgrad_nsplit',
                                                          'wgrad_rows_per_split']),
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
        assert [k for k, _ in ct._fields_] == fields
        for f in fields:
            assert int(got['%s.%s' % (name, f)]) == getattr(ct, f).offset, (name, f)
    assert int(got['abi']) == 6
    assert C.sizeof(_lib.NodeBnMiniStemInfo) == 28


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_and_taken_shapes():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    St = _lib.NodeMiniStemShape
    size = lambda s, keep: lib.node_bnministem_workspace_bytes(C.byref(s), keep)
    info = (_lib.NodeBnMiniStemInfo * 2)()
    for bad, word, code in ((St(2, 4, 32, 32, 64, 1e-5), 'in_ch', NODE_ERR_UNSUPPORTED), (St(2, 3, 32, 32, 96, 1e-5), 'power of two', NODE_ERR_UNSUPPORTED),
                            (St(2, 3, 32, 32, 24, 1e-5), 'power of two', NODE_ERR_UNSUPPORTED), (St(2, 3, 32, 32, 8192, 1e-5), 'power of two', NODE_ERR_UNSUPPORTED),
                            (St(2, 3, 9, 32, 64, 1e-5), '10 x 10', NODE_ERR_SHAPE), (St(2, 3, 32, 9, 64, 1e-5), '10 x 10', NODE_ERR_SHAPE),
                            (St(100000, 3, 32, 32, 64, 1e-5), '2^31', NODE_ERR_UNSUPPORTED), (St(2048, 3, 32, 32, 4096, 1e-5), '2^31', NODE_ERR_UNSUPPORTED),
                            (St(0, 3, 32, 32, 64, 1e-5), 'shape', NODE_ERR_SHAPE)):
        for keep in (0, 1):
            assert size(bad, keep) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_bnministem_fwd(C.byref(bad), None, None, None, 1, None, 0, None) == code
        assert lib.node_bnministem_bwd(C.byref(bad), None, None, None, None, None, None, 0, None) == code
        assert lib.node_bnministem_describe(C.byref(bad), info) == code
        # the GroupNorm stem refuses the same shapes with the same words
        assert lib.node_ministem_workspace_bytes(C.byref(bad), 1) == 0 and word in lib.node_last_error().decode()
    assert size(St(1, 1, 10, 10, 64, 1e-5), 1) > size(St(1, 1, 10, 10, 64, 1e-5), 0) > 0      # the floor
    assert size(St(128, 3, 32, 32, 256, 1e-5), 1) < (1 << 28)
    assert size(St(2, 3, 64, 64, 64, 1e-5), 1) > 0                       # no limit on the image: no pass holds a plane
    assert lib.node_bnministem_workspace_bytes(None, 1) == 0
    assert lib.node_bnministem_describe(C.byref(St(2, 3, 32, 32, 64, 1e-5)), None) == NODE_ERR_NULL
    assert lib.node_bnministem_describe(None, info) == NODE_ERR_NULL
    with pytest.raises(_lib.NodeHipError, match='power of two'):
        _lib.bnministem_plan(2, 3, 32, 32, 96)


def tensors_of(case):
    """rows of the two normalised tensors h0, h1"""
    n, _, h, w = K.shape_of(case)
    h0, w0 = h - 2, w - 2
    return [n * h0 * w0, n * K._out4(h0) * K._out4(w0)]


@pytest.mark.parametrize('case', K.ALL_CASES + [(3, 32, 256, 128), (3, 64, 64, 64)], ids=_id)
def test_every_case_has_a_workspace_and_the_plan_of_the_chunk_function(case):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    n, cin, h, w = K.shape_of(case)
    s = _lib.NodeMiniStemShape(n, cin, h, w, case[2], 1e-5)
    keep, scratch = lib.node_bnministem_workspace_bytes(C.byref(s), 1), lib.node_bnministem_workspace_bytes(C.byref(s), 0)
    assert 0 < scratch < keep
    plan = K.plan_of(case)
    assert len(plan) == 2
    for d, rows in zip(plan, tensors_of(case)):
        cr = chunk_rows(rows)
        nchunk = -(-rows // cr)
        assert (d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows'], d['trip_rows']) == (rows, cr, nchunk, rows - (nchunk - 1) * cr, TRIP), (case, d)
        assert 1 <= d['nchunk'] <= MAX_CHUNKS and d['chunk_rows'] % d['trip_rows'] == 0 and 1 <= d['last_chunk_rows'] <= d['chunk_rows']
        assert d['wgrad_nsplit'] >= 1 and d['wgrad_rows_per_split'] % 32 == 0


def test_the_cap_of_the_environment_changes_the_plan_and_the_workspace(monkeypatch):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    s = _lib.NodeMiniStemShape(128, 3, 32, 32, 256, 1e-5)
    base = lib.node_bnministem_workspace_bytes(C.byref(s), 1)
    for cap in (64, 256, 1024):
        monkeypatch.setenv(ENV, str(cap))
        for d in _lib.bnministem_plan(128, 3, 32, 32, 256):
            cr = chunk_rows(d['rows'], cap)
            assert (d['chunk_rows'], d['nchunk']) == (cr, -(-d['rows'] // cr)) and d['nchunk'] <= cap
        assert (lib.node_bnministem_workspace_bytes(C.byref(s), 1) > base) == (cap > MAX_CHUNKS)
    monkeypatch.setenv(ENV, '0')
    assert lib.node_bnministem_workspace_bytes(C.byref(s), 1) == base


def test_the_cases_reach_their_regimes():
    """A later change of the chunk heuristics cannot quietly empty these cases."""
    reached = set()
    for case, asked in K.MULTI.items():
        assert case in K.ALL_CASES
        plan = K.plan_of(case)
        for norm, regime in asked:
            assert K.REGIMES[regime](plan[norm]), (case, norm, regime, plan[norm])
            reached.add(regime)
    assert reached == set(K.REGIMES)                                     # every regime has a case and a norm
    plan = K.plan_of((3, 32, 64, 5))
    assert [(d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows']) for d in plan] == [(4500, 64, 71, 20), (1125, 32, 36, 5)]
    plan = K.plan_of((1, 10, 64, 1))
    assert [(d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows']) for d in plan] == [(64, 32, 2, 32), (16, 32, 1, 16)]
    # the timing shape: 29 trips a chunk
    plan = K.plan_of((3, 32, 256, 128))
    assert [(d['rows'], d['chunk_rows'], d['nchunk']) for d in plan] == [(115200, 928, 125), (28800, 256, 113)]


def _host_buffer():
    buf = (C.c_char * 16384)()
    return buf, (C.addressof(buf) + 255) & ~255


def test_null_misaligned_and_short_workspace_arguments_are_rejected_before_any_launch():
    """Every call below returns before its first launch (this test runs without a GPU); the pointers are host memory that is
    never read."""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeMiniStemShape(2, 3, 32, 32, 64, 1e-5)
    s = C.byref(shape)
    nbytes = lib.node_bnministem_workspace_bytes(s, 1)
    buf, base = _host_buffer()
    P = _lib.NodeMiniStemParams

    def tensors(hole=None, odd=None):
        vals = [base + 256 * k for k in range(10)]
        if hole is not None:
            vals[hole] = None
        if odd is not None:
            vals[odd] += 4
        return C.byref(P(*vals))
    good = tensors()
    x, out, ws = base + 4352, base + 4608, base + 4864
    fwd, bwd = lib.node_bnministem_fwd, lib.node_bnministem_bwd
    assert fwd(None, good, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, None, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, tensors(hole=9), x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, tensors(odd=2), x, out, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert 'aligned' in lib.node_last_error().decode()
    assert fwd(s, good, None, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, out, 1, None, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, out, 1, ws + 16, nbytes, None) == NODE_ERR_ARG
    assert '256-byte' in lib.node_last_error().decode()
    assert fwd(s, good, x, out, 1, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    assert 'too small' in lib.node_last_error().decode()
    assert fwd(s, good, x, out, 0, ws, lib.node_bnministem_workspace_bytes(s, 0) - 1, None) == NODE_ERR_WORKSPACE
    for grads, d_x in ((good, x), (good, None), (None, x)):
        assert bwd(None, good, x, out, grads, d_x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, None, x, out, grads, d_x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, tensors(hole=0), x, out, grads, d_x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, tensors(odd=3), x, out, grads, d_x, ws, nbytes, None) == NODE_ERR_ARG
        assert bwd(s, good, None, out, grads, d_x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, good, x, None, grads, d_x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, good, x, out, grads, d_x, None, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, good, x, out, grads, d_x, ws + 16, nbytes, None) == NODE_ERR_ARG
        assert bwd(s, good, x, out, grads, d_x, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
        assert 'too small' in lib.node_last_error().decode()
    assert bwd(s, good, x, out, None, None, ws, nbytes, None) == NODE_ERR_NULL
    assert 'both NULL' in lib.node_last_error().decode()
    assert bwd(s, good, x, out, tensors(hole=5), x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, out, tensors(odd=9), x, ws, nbytes, None) == NODE_ERR_ARG
    del buf


# ---------------------------------------------------------------------------------------------------------------------
# recognition, the CPU path
# ---------------------------------------------------------------------------------------------------------------------
def _stem(filters=64, in_ch=3, norm='batch'):
    import neural_ode_features_amd as nof
    return nof.ODENet(in_ch, out=10, n_filters=filters, downsample='minimal', adjoint=True, norm=norm).downsample.module


def test_recognition_of_stems():
    from neural_ode_features_amd import ministem
    s = _stem(256)
    assert isinstance(s, ministem.MinimalStem) and isinstance(s[1], nn.BatchNorm2d)
    ps = ministem._bn_params_of(s)
    assert ps is not None and len(ps) == 10
    assert [tuple(p.shape) for p in ps] == [(24, 3, 3, 3), (24,), (24,), (24,), (24, 24, 4, 4), (24,), (24,), (24,), (256, 24, 4, 4), (256,)]
    assert [id(p) for p in ps] == [id(p) for p in s.parameters()]                    # state_dict order
    assert ministem._params_of(s) is None                                            # GroupNorm only, as it was
    gn = _stem(norm='group')
    assert len(ministem._params_of(gn)) == 10 and ministem._bn_params_of(gn) is None
    assert ministem.MinimalStem.fused_batch is False and ministem.MinimalStem.input_grad is False      # (the timing run decided: README)
    # running statistics, no affine parameters, another eps in one slot, GroupNorm children, another geometry, no bias: the module sequence
    tracked = _stem()
    tracked[4] = nn.BatchNorm2d(24)
    assert ministem._bn_params_of(tracked) is None
    plain = _stem()
    plain[1] = nn.BatchNorm2d(24, affine=False, track_running_stats=False)
    assert ministem._bn_params_of(plain) is None
    eps = _stem()
    eps[4].eps = 1e-3
    assert ministem._bn_params_of(eps) is None
    mixed = _stem()
    mixed[4] = nn.GroupNorm(24, 24)
    assert ministem._bn_params_of(mixed) is None and ministem._params_of(mixed) is None
    wrong = _stem()
    wrong[3] = nn.Conv2d(24, 24, 3, 2, 1)
    assert ministem._bn_params_of(wrong) is None
    wide = _stem()
    wide[1] = nn.BatchNorm2d(32, track_running_stats=False)
    assert ministem._bn_params_of(wide) is None
    nobias = _stem()
    nobias[6] = nn.Conv2d(24, 64, 4, 2, 1, bias=False)
    assert ministem._bn_params_of(nobias) is None
    assert ministem._bn_params_of(nn.Sequential(*list(_stem())[:5])) is None
    # filters = 96 is recognised as a stem and refused by shape (bn_fusable needs a HIP tensor: a CPU tensor is refused first)
    assert ministem._bn_params_of(_stem(96)) is not None
    assert not ministem.bn_fusable(s, torch.randn(2, 3, 32, 32))
    assert not ministem.bn_fusable(s, torch.randn(2, 3, 32, 32), input_grad=True)
    # hooks on a sub-module send the stem to the modules; a hook on the stem itself does not
    hooked = _stem()
    handle = hooked[1].register_forward_hook(lambda m, i, o: None)
    assert ministem._hooked(hooked)
    handle.remove()
    handle = hooked.register_forward_hook(lambda m, i, o: None)
    assert not ministem._hooked(hooked)
    handle.remove()


@pytest.mark.parametrize('training', [True, False])
def test_cpu_stem_is_the_module_sequence_bit_for_bit(training):
    s = _stem()
    s.train(training)
    x = torch.randn(2, 3, 32, 32).requires_grad_(True)
    out, want = s(x), nn.Sequential.forward(s, x)
    assert type(out.grad_fn).__name__ != '_BnMiniStemFnBackward'
    assert torch.equal(out, want)
    g, gw = torch.autograd.grad(out, [x] + list(s.parameters()), torch.ones_like(out)), torch.autograd.grad(want, [x] + list(s.parameters()), torch.ones_like(out))
    for u, v in zip(g, gw):
        assert torch.equal(u, v)
    assert not any('running' in k for k in s.state_dict())


# ---------------------------------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in K.ALL_CASES if c in K.SEEDS], ids=_id)
def test_seeds_of_the_gpu_cases_keep_every_relu_mask(case):
    """The seeds the GPU tests run their ordinary-parameter cases with: every ReLU mask of the fp32 CPU run agrees with the fp64
    run's, at a margin ratio no smaller than the yardstick's (bnministem_cases.py has the recipe)."""
    agree, margin, ratio = K.margin_ratio(case, K.SEEDS[case])
    assert agree and margin > 0
    assert ratio >= B.margin_ratio(*B.RATIO_YARDSTICK)[2], (case, ratio)


@pytest.mark.parametrize('mode', ['kinkfree', 'split'])
@pytest.mark.parametrize('case', K.ALL_CASES, ids=_id)
def test_kinkfree_and_split_sets_have_no_kink(case, mode):
    constant, margin = K.sign_condition(case, mode)
    assert constant and margin > 0.5, (case, mode, margin)


def test_every_case_runs_every_mode():
    assert [c for c in K.ALL_CASES if c not in K.SEEDS] == []
    for case in K.ALL_CASES:
        assert [m for _, m in K.runs(case)] == list(K.MODES)

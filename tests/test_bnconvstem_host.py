"""Host side (no GPU) of the `norm='batch'` convolution stem (convstem.py `_BnConvStemFn`, csrc/bnconvstem_api.hip) and of the `ode2`
stem's `norm='batch'` hand-off (downconv.py `_BnDownConvFn`, csrc/bndownconv_api.hip): the ABI and the layouts of its structures, the
launch plans of the cases tests/test_gpu_bnconvstem.py and tests/test_gpu_bndownconv.py run (through the two describe calls; the sliced
plan among them), the argument checks of the C ABI -- every one of which returns before a launch --, what the Python layer
recognises and refuses, the CPU paths, and the seeds."""
import ctypes as C
import os
import subprocess

import pytest
import torch
from torch import nn

from tests import bnconvstem_cases as K
from tests import bnfunc_cases as B

NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED, NODE_ERR_WORKSPACE, NODE_ERR_ARG = -1, -2, -3, -4, -9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = 'NODE_TUNE_BNSTEM_MAXCHUNK'
STEM_CALLS = ('node_bnconvstem_workspace_bytes', 'node_bnconvstem_describe', 'node_bnconvstem_fwd', 'node_bnconvstem_bwd', 'node_bnconvstem_bwd_dx')
DOWN_CALLS = ('node_bndownconv_workspace_bytes', 'node_bndownconv_describe', 'node_bndownconv_fwd', 'node_bndownconv_bwd')


def chunk_rows(rows, c, cap=128):
    """bnstem_chunk_rows of csrc/bnstem_api.hip, restated: at most `cap` chunks at C = 64, 2 cap / (C / 64) for wider tensors (never
    under 16), whole 32-row trips."""
    maxchunk = max(16, min(cap, 2 * cap // (c // 64)))
    cr = -(-rows // maxchunk)
    return max(32, (cr + 31) & ~31)


def _id(case):
    return '_'.join('%dx%d' % v if isinstance(v, tuple) else str(v) for v in case)


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)


def test_exports_and_abi_version():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in STEM_CALLS + DOWN_CALLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additions only
    header = open(os.path.join(ROOT, 'include', 'node_hip.h')).read()
    for proto in ('size_t node_bnconvstem_workspace_bytes(const node_convstem_shape* shape, int keep_for_backward);',
                  'int node_bnconvstem_describe(const node_convstem_shape* shape, node_bnfunc_info out[2]);',
                  'size_t node_bndownconv_workspace_bytes(const node_bndownconv_shape* shape, int keep_for_backward);',
                  'int node_bndownconv_describe(const node_bndownconv_shape* shape, node_bnfunc_info* out);'):
        assert proto in header


def test_ctypes_layouts_match_the_header(tmp_path):
    """The gcc `offsetof` program of tests/test_ministem_host.py for the structures these calls take; the version stays 6."""
    from neural_ode_features_amd import _lib
    structs = {
        'node_bndownconv_shape': (_lib.NodeBnDownConvShape, ['n', 'cin', 'cout', 'h', 'w', 'slices', 'eps']),
        'node_convstem_shape': (_lib.NodeConvStemShape, ['n', 'in_ch', 'h', 'w', 'filters', 'eps']),
        'node_convstem_params': (_lib.NodeConvStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
        'node_convstem_grads': (_lib.NodeConvStemParams, list(_lib.CONVSTEM_PARAM_FIELDS)),
        'node_downconv_params': (_lib.NodeDownConvParams, list(_lib.DOWNCONV_PARAM_FIELDS)),
        'node_downconv_grads': (_lib.NodeDownConvParams, list(_lib.DOWNCONV_PARAM_FIELDS)),
        'node_bnfunc_info': (_lib.NodeBnfuncInfo, [k for k, _ in _lib.NodeBnfuncInfo._fields_]),
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
    assert C.sizeof(_lib.NodeBnDownConvShape) == 28


# ---------------------------------------------------------------------------------------------------------------------
# the stem's C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_stem_refused_and_taken_shapes():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    St = _lib.NodeConvStemShape
    size = lambda s, keep: lib.node_bnconvstem_workspace_bytes(C.byref(s), keep)
    info = (_lib.NodeBnfuncInfo * 2)()
    for bad, word, code in ((St(2, 4, 32, 32, 64, 1e-5), 'in_ch', NODE_ERR_UNSUPPORTED), (St(2, 3, 32, 32, 96, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED),
                            (St(2, 3, 32, 32, 32, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED), (St(2, 3, 32, 32, 8192, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED),
                            (St(2, 3, 9, 32, 64, 1e-5), '10 x 10', NODE_ERR_SHAPE), (St(2, 3, 32, 9, 64, 1e-5), '10 x 10', NODE_ERR_SHAPE),
                            (St(2, 3, 64, 64, 64, 1e-5), '2400', NODE_ERR_UNSUPPORTED), (St(20000, 3, 50, 50, 64, 1e-5), '2^31', NODE_ERR_UNSUPPORTED),
                            (St(0, 3, 32, 32, 64, 1e-5), 'shape', NODE_ERR_SHAPE)):
        for keep in (0, 1):
            assert size(bad, keep) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_bnconvstem_fwd(C.byref(bad), None, None, None, 1, None, 0, None) == code
        assert lib.node_bnconvstem_bwd(C.byref(bad), None, None, None, None, None, 0, None) == code
        assert lib.node_bnconvstem_bwd_dx(C.byref(bad), None, None, None, None, None, None, 0, None) == code
        assert lib.node_bnconvstem_describe(C.byref(bad), info) == code
    assert size(St(1, 1, 10, 10, 64, 1e-5), 1) > 0                       # the floor
    assert size(St(128, 3, 32, 32, 256, 1e-5), 1) < (1 << 30)
    for filters in (192, 384):                                           # BatchNorm has no groups: what the GroupNorm stem refuses
        assert lib.node_convstem_workspace_bytes(C.byref(St(2, 3, 32, 32, filters, 1e-5)), 1) == 0
        assert size(St(2, 3, 32, 32, filters, 1e-5), 1) > 0
    assert lib.node_bnconvstem_workspace_bytes(None, 1) == 0
    assert lib.node_bnconvstem_describe(C.byref(St(2, 3, 32, 32, 64, 1e-5)), None) == NODE_ERR_NULL
    assert lib.node_bnconvstem_describe(None, info) == NODE_ERR_NULL


def stem_tensors_of(case):
    """(rows, channels) of the two normalised tensors h0, h1"""
    n, _, h, w = K.shape_of(case)
    h0, w0 = h - 2, w - 2
    return [(n * h0 * w0, 64), (n * K._out4(h0) * K._out4(w0), 64)]


@pytest.mark.parametrize('case', K.STEM_ALL, ids=_id)
def test_every_stem_case_has_a_workspace_and_the_plan_of_the_chunk_function(case, monkeypatch):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    n, cin, h, w = K.shape_of(case)
    s = _lib.NodeConvStemShape(n, cin, h, w, case[3], 1e-5)
    keep, scratch = lib.node_bnconvstem_workspace_bytes(C.byref(s), 1), lib.node_bnconvstem_workspace_bytes(C.byref(s), 0)
    assert 0 < scratch < keep
    for cap in (128, 1024):
        monkeypatch.setenv(ENV, str(cap))                                # these are stem tensors: the stems' cap applies
        plan = _lib.bnconvstem_plan(n, cin, h, w, case[3])
        assert len(plan) == 2
        for d, (rows, c) in zip(plan, stem_tensors_of(case)):
            cr = chunk_rows(rows, c, cap)
            nchunk = -(-rows // cr)
            assert (d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows'], d['column_tiles']) == (rows, cr, nchunk, rows - (nchunk - 1) * cr, 1), (case, d)
            assert d['wgrad_nsplit'] >= 1 and d['wgrad_rows_per_split'] % 16 == 0


def test_small_stem_cases_run_one_trip_and_the_multi_chunk_case_reaches_its_regimes():
    """A later change of the chunk or split heuristics cannot quietly empty these cases."""
    from neural_ode_features_amd import _lib
    for case in K.STEM_CASES:
        n, cin, h, w = K.shape_of(case)
        for d in _lib.bnconvstem_plan(n, cin, h, w, case[3]):
            assert d['chunk_rows'] == 32 and d['nchunk'] == -(-d['rows'] // 32), (case, d)
    assert _lib.bnconvstem_plan(1, 1, 10, 10, 64)[1]['rows'] == 16       # ... and 2 x 2 = four values per channel behind the last convolution
    for case, asked in K.STEM_MULTI.items():
        n, cin, h, w = K.shape_of(case)
        plan = _lib.bnconvstem_plan(n, cin, h, w, case[3])
        for norm, regime in asked:
            assert K.REGIMES[regime](plan[norm]), (case, norm, regime, plan[norm])
        assert [(d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows']) for d in plan] == [(4500, 64, 71, 20), (1125, 32, 36, 5)]


def _host_buffer():
    buf = (C.c_char * 16384)()
    return buf, (C.addressof(buf) + 255) & ~255


def test_stem_null_misaligned_and_short_workspace_arguments_are_rejected_before_any_launch():
    """Every call below returns before its first launch (this test runs without a GPU); the pointers are host memory that is
    never read."""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeConvStemShape(2, 3, 32, 32, 64, 1e-5)
    s = C.byref(shape)
    nbytes = lib.node_bnconvstem_workspace_bytes(s, 1)
    buf, base = _host_buffer()
    P = _lib.NodeConvStemParams

    def tensors(hole=None, odd=None):
        vals = [base + 256 * k for k in range(10)]
        if hole is not None:
            vals[hole] = None
        if odd is not None:
            vals[odd] += 4
        return C.byref(P(*vals))
    good = tensors()
    x, out, ws = base + 4352, base + 4608, base + 4864
    fwd, bwd, bwd_dx = lib.node_bnconvstem_fwd, lib.node_bnconvstem_bwd, lib.node_bnconvstem_bwd_dx
    assert fwd(None, good, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, None, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, tensors(hole=9), x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, tensors(odd=2), x, out, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, None, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x + 4, out, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out + 8, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out, 1, None, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, out, 1, ws + 16, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out, 1, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    assert 'too small' in lib.node_last_error().decode()
    assert fwd(s, good, x, out, 0, ws, lib.node_bnconvstem_workspace_bytes(s, 0) - 1, None) == NODE_ERR_WORKSPACE
    # node_bnconvstem_bwd: grads required
    assert bwd(None, good, x, out, good, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, None, x, out, good, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, tensors(hole=0), x, out, good, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, None, out, good, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, None, good, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, out + 4, good, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, out, None, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, out, tensors(hole=5), ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, out, tensors(odd=9), ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, out, good, None, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, out, good, ws + 16, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, out, good, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    # node_bnconvstem_bwd_dx: d_x required, grads nullable
    assert bwd_dx(s, good, x, out, good, None, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd_dx(s, good, x, out, None, None, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd_dx(s, good, x, out, None, x + 8, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd_dx(s, good, x, out, tensors(hole=5), x, ws, nbytes, None) == NODE_ERR_NULL
    for grads in (good, None):
        assert bwd_dx(s, tensors(odd=1), x, out, grads, x, ws, nbytes, None) == NODE_ERR_ARG
        assert bwd_dx(s, good, x, out, grads, x, None, nbytes, None) == NODE_ERR_NULL
        assert bwd_dx(s, good, x, out, grads, x, ws + 16, nbytes, None) == NODE_ERR_ARG
        assert bwd_dx(s, good, x, out, grads, x, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    del buf


# ---------------------------------------------------------------------------------------------------------------------
# the hand-off's C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_handoff_refused_and_taken_shapes():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    Sh = _lib.NodeBnDownConvShape
    size = lambda s, keep: lib.node_bndownconv_workspace_bytes(C.byref(s), keep)
    info = _lib.NodeBnfuncInfo()
    for bad, word, code in ((Sh(2, 96, 64, 8, 8, 1, 1e-5), 'multiples of 64', NODE_ERR_UNSUPPORTED), (Sh(2, 64, 32, 8, 8, 1, 1e-5), 'multiples of 64', NODE_ERR_UNSUPPORTED),
                            (Sh(2, 8192, 64, 8, 8, 1, 1e-5), 'multiples of 64', NODE_ERR_UNSUPPORTED), (Sh(2, 64, 64, 3, 8, 1, 1e-5), '4x4', NODE_ERR_SHAPE),
                            (Sh(2, 64, 64, 8, 3, 1, 1e-5), '4x4', NODE_ERR_SHAPE), (Sh(0, 64, 64, 8, 8, 1, 1e-5), 'shape', NODE_ERR_SHAPE),
                            (Sh(6, 64, 64, 8, 8, 4, 1e-5), 'slices', NODE_ERR_SHAPE), (Sh(6, 64, 64, 8, 8, 0, 1e-5), 'slices', NODE_ERR_SHAPE),
                            (Sh(6, 64, 64, 8, 8, -1, 1e-5), 'slices', NODE_ERR_SHAPE), (Sh(40000, 256, 256, 16, 16, 1, 1e-5), '2^31', NODE_ERR_UNSUPPORTED)):
        for keep in (0, 1):
            assert size(bad, keep) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_bndownconv_fwd(C.byref(bad), None, None, None, 0, None, 0, None) == code
        assert lib.node_bndownconv_bwd(C.byref(bad), None, None, None, None, None, 0, None) == code
        assert lib.node_bndownconv_describe(C.byref(bad), C.byref(info)) == code
    # slices > 1 is the forward without a backward to come
    sl = Sh(6, 64, 64, 8, 8, 3, 1e-5)
    assert size(sl, 0) > 0 and size(sl, 1) == 0
    assert 'keep_for_backward = 0 only' in lib.node_last_error().decode()
    assert lib.node_bndownconv_fwd(C.byref(sl), None, None, None, 1, None, 0, None) == NODE_ERR_UNSUPPORTED
    assert lib.node_bndownconv_bwd(C.byref(sl), None, None, None, None, None, 0, None) == NODE_ERR_UNSUPPORTED
    assert lib.node_bndownconv_fwd(C.byref(sl), None, None, None, 0, None, 0, None) == NODE_ERR_NULL      # (taken: the next check is the parameters')
    assert lib.node_bndownconv_describe(C.byref(sl), C.byref(info)) == 0
    # what the GroupNorm hand-off refuses: 192 channels, an image that does not fit an LDS block
    for shape6, shape7 in (((2, 192, 192, 8, 8), (2, 192, 192, 8, 8, 1)), ((2, 256, 256, 64, 64), (2, 256, 256, 64, 64, 1))):
        assert lib.node_downconv_workspace_bytes(C.byref(_lib.NodeDownConvShape(*shape6, 1e-5)), 1) == 0
        assert size(Sh(*shape7, 1e-5), 1) > 0
    assert size(Sh(2, 64, 64, 4, 4, 1, 1e-5), 1) > size(Sh(2, 64, 64, 4, 4, 1, 1e-5), 0) > 0       # the floor
    assert lib.node_bndownconv_workspace_bytes(None, 1) == 0
    assert lib.node_bndownconv_describe(C.byref(sl), None) == NODE_ERR_NULL
    assert lib.node_bndownconv_describe(None, C.byref(info)) == NODE_ERR_NULL


@pytest.mark.parametrize('case', K.DOWN_ALL, ids=_id)
def test_every_handoff_case_has_a_workspace_and_the_plan_of_the_chunk_function(case):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    _, n, cin, cout, _ = case
    _, _, h, w = K.shape_of(case)
    s = _lib.NodeBnDownConvShape(n, cin, cout, h, w, 1, 1e-5)
    assert 0 < lib.node_bndownconv_workspace_bytes(C.byref(s), 0) < lib.node_bndownconv_workspace_bytes(C.byref(s), 1)
    d = _lib.describe_bndownconv(n, cin, cout, h, w)
    rows = n * h * w
    cr = chunk_rows(rows, cin)
    nchunk = -(-rows // cr)
    assert (d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows'], d['column_tiles']) == (rows, cr, nchunk, rows - (nchunk - 1) * cr, cin // 64)
    assert d['wgrad_nsplit'] >= 1 and d['wgrad_rows_per_split'] % 16 == 0
    if case in K.DOWN_MULTI:
        for regime in K.DOWN_MULTI[case]:
            assert K.REGIMES[regime](d), (case, regime, d)
        assert (d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows']) == (4104, 64, 65, 8)
    else:
        assert d['chunk_rows'] == 32


@pytest.mark.parametrize('shape', [(3, 2, 64, 8, 8), (3, 2, 64, 7, 6), (21, 128, 256, 16, 16), (5, 9, 64, 24, 19), (4, 3, 192, 9, 5)])
def test_a_sliced_plan_is_the_single_slice_plan_once_per_slice(shape, monkeypatch):
    """chunk_rows = what a call on one slice alone takes (so every slice has the bits of its own call), nchunk = slices x chunks per
    slice, last_chunk_rows = the last chunk's of every slice; under the stems' cap as well."""
    from neural_ode_features_amd import _lib
    t, n, c, h, w = shape
    for cap in (None, 1024):
        if cap:
            monkeypatch.setenv(ENV, str(cap))
        one = _lib.describe_bndownconv(n, c, c, h, w)
        all_ = _lib.describe_bndownconv(t * n, c, c, h, w, slices=t)
        flat = _lib.describe_bndownconv(t * n, c, c, h, w)
        assert all_['chunk_rows'] == one['chunk_rows'] == chunk_rows(n * h * w, c, cap or 128)
        assert all_['nchunk'] == t * one['nchunk'] and all_['last_chunk_rows'] == one['last_chunk_rows']
        assert all_['rows'] == t * one['rows'] == flat['rows'] and all_['column_tiles'] == c // 64
    monkeypatch.delenv(ENV)
    d = _lib.describe_bndownconv(6, 64, 64, 7, 6, slices=3)       # 84 rows per slice: chunks of 32, 32 and 20 rows, three times
    assert (d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows']) == (252, 32, 9, 20)
    with pytest.raises(_lib.NodeHipError, match='slices'):
        _lib.describe_bndownconv(7, 64, 64, 8, 8, slices=3)


def test_handoff_null_misaligned_and_short_workspace_arguments_are_rejected_before_any_launch():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    buf, base = _host_buffer()
    P = _lib.NodeDownConvParams

    def tensors(hole=None, odd=None):
        vals = [base + 256 * k for k in range(4)]
        if hole is not None:
            vals[hole] = None
        if odd is not None:
            vals[odd] += 4
        return C.byref(P(*vals))
    good = tensors()
    x, y, ws = base + 4352, base + 4608, base + 4864
    fwd, bwd = lib.node_bndownconv_fwd, lib.node_bndownconv_bwd
    for slices, keep in ((1, 1), (1, 0), (3, 0)):
        shape = _lib.NodeBnDownConvShape(6, 64, 128, 8, 8, slices, 1e-5)
        s = C.byref(shape)
        nbytes = lib.node_bndownconv_workspace_bytes(s, keep)
        assert nbytes > 0
        assert fwd(None, good, x, y, keep, ws, nbytes, None) == NODE_ERR_NULL
        assert fwd(s, None, x, y, keep, ws, nbytes, None) == NODE_ERR_NULL
        assert fwd(s, tensors(hole=3), x, y, keep, ws, nbytes, None) == NODE_ERR_NULL
        assert fwd(s, tensors(odd=0), x, y, keep, ws, nbytes, None) == NODE_ERR_ARG
        assert fwd(s, good, None, y, keep, ws, nbytes, None) == NODE_ERR_NULL
        assert fwd(s, good, x, None, keep, ws, nbytes, None) == NODE_ERR_NULL
        assert fwd(s, good, x + 4, y, keep, ws, nbytes, None) == NODE_ERR_ARG
        assert fwd(s, good, x, y + 8, keep, ws, nbytes, None) == NODE_ERR_ARG
        assert fwd(s, good, x, y, keep, None, nbytes, None) == NODE_ERR_NULL
        assert fwd(s, good, x, y, keep, ws + 16, nbytes, None) == NODE_ERR_ARG
        assert fwd(s, good, x, y, keep, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
        assert 'too small' in lib.node_last_error().decode()
    assert fwd(s, good, x, y, 1, ws, 1 << 40, None) == NODE_ERR_UNSUPPORTED               # slices = 3 with a backward to come
    assert bwd(s, good, y, good, x, ws, 1 << 40, None) == NODE_ERR_UNSUPPORTED
    shape = _lib.NodeBnDownConvShape(6, 64, 128, 8, 8, 1, 1e-5)
    s = C.byref(shape)
    nbytes = lib.node_bndownconv_workspace_bytes(s, 1)
    for grads in (good, None):
        assert bwd(None, good, y, grads, x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, None, y, grads, x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, tensors(hole=1), y, grads, x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, tensors(odd=2), y, grads, x, ws, nbytes, None) == NODE_ERR_ARG
        assert bwd(s, good, None, grads, x, ws, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, good, y + 4, grads, x, ws, nbytes, None) == NODE_ERR_ARG
        assert bwd(s, good, y, grads, None, ws, nbytes, None) == NODE_ERR_NULL            # d_x is required
        assert bwd(s, good, y, grads, x + 8, ws, nbytes, None) == NODE_ERR_ARG
        assert bwd(s, good, y, grads, x, None, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, good, y, grads, x, ws + 16, nbytes, None) == NODE_ERR_ARG
        assert bwd(s, good, y, grads, x, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    assert bwd(s, good, y, tensors(hole=2), x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, y, tensors(odd=3), x, ws, nbytes, None) == NODE_ERR_ARG
    del buf


# ---------------------------------------------------------------------------------------------------------------------
# recognition, the CPU paths
# ---------------------------------------------------------------------------------------------------------------------
def _stem(filters=64, in_ch=3, norm='batch'):
    import neural_ode_features_amd as nof
    return nof.ODENet(in_ch, out=10, n_filters=filters, downsample='convolution', adjoint=True, norm=norm).downsample.module


def test_recognition_of_stems():
    from neural_ode_features_amd import convstem
    s = _stem(192)
    assert isinstance(s, convstem.ConvStem) and convstem._is_batch(s)
    ps = convstem._bn_params_of(s)
    assert ps is not None and len(ps) == 10
    assert [tuple(p.shape) for p in ps] == [(64, 3, 3, 3), (64,), (64,), (64,), (64, 64, 4, 4), (64,), (64,), (64,), (192, 64, 4, 4), (192,)]
    assert [id(p) for p in ps] == [id(p) for p in s.parameters()]                    # state_dict order
    assert convstem._params_of(s) is None                                            # GroupNorm only, as it was
    gn = _stem(norm='group')
    assert len(convstem._params_of(gn)) == 10 and convstem._bn_params_of(gn) is None and not convstem._is_batch(gn)
    assert convstem.ConvStem.fused_batch is True and convstem.ConvStem.input_grad is False
    # running statistics, no affine parameters, another eps in one slot, a GroupNorm in one slot, another geometry: the module sequence
    tracked = _stem()
    tracked[4] = nn.BatchNorm2d(64)
    assert convstem._bn_params_of(tracked) is None
    plain = _stem()
    plain[1] = nn.BatchNorm2d(64, affine=False, track_running_stats=False)
    assert convstem._bn_params_of(plain) is None
    eps = _stem()
    eps[4].eps = 1e-3
    assert convstem._bn_params_of(eps) is None
    mixed = _stem()
    mixed[4] = nn.GroupNorm(32, 64)
    assert convstem._bn_params_of(mixed) is None and convstem._params_of(mixed) is None
    wrong = _stem()
    wrong[3] = nn.Conv2d(64, 64, 3, 2, 1)
    assert convstem._bn_params_of(wrong) is None
    nobias = _stem()
    nobias[6] = nn.Conv2d(64, 64, 4, 2, 1, bias=False)
    assert convstem._bn_params_of(nobias) is None
    # filters = 96 is recognised as a stem and refused by shape (bn_fusable needs a HIP tensor: a CPU tensor is refused first)
    assert convstem._bn_params_of(_stem(96)) is not None
    assert not convstem.bn_fusable(s, torch.randn(2, 3, 32, 32))
    # hooks on a sub-module send the stem to the modules; a hook on the stem itself does not
    hooked = _stem()
    handle = hooked[1].register_forward_hook(lambda m, i, o: None)
    assert convstem._hooked(hooked)
    handle.remove()
    handle = hooked.register_forward_hook(lambda m, i, o: None)
    assert not convstem._hooked(hooked)
    handle.remove()
    # the minimal stem stays what it was: 24 channels do not fit the 64-channel BatchNorm workgroups
    import neural_ode_features_amd as nof
    mini = nof.ODENet(3, out=10, n_filters=64, downsample='minimal', adjoint=True, norm='batch').downsample.module
    assert not isinstance(mini, convstem.ConvStem)


def test_recognition_of_handoffs():
    from neural_ode_features_amd import downconv
    bn, conv = nn.BatchNorm2d(64, track_running_stats=False), nn.Conv2d(64, 64, 4, 2, 1)
    x = torch.randn(2, 64, 8, 8)
    assert not downconv.bn_fusable(x, bn, conv) and not downconv.fusable(x, bn, conv)      # a CPU tensor is refused first
    assert not downconv._hooked(bn, conv)
    handle = conv.register_forward_hook(lambda m, i, o: None)
    assert downconv._hooked(bn, conv)
    handle.remove()
    # the modules on the CPU, bit for bit: unsliced, and sliced = slice by slice (NOT the flattened batch)
    want = conv(torch.relu(bn(x)))
    assert torch.equal(downconv.bn_relu_conv(x, bn, conv), want)
    traj = torch.randn(3, 2, 64, 8, 8)
    got = downconv.bn_relu_conv(traj.reshape(6, 64, 8, 8), bn, conv, slices=3)
    assert torch.equal(got, torch.cat([conv(torch.relu(bn(xi))) for xi in traj]))
    assert not torch.equal(got, downconv.bn_relu_conv(traj.reshape(6, 64, 8, 8), bn, conv))


@pytest.mark.parametrize('training', [True, False])
def test_cpu_stem_is_the_module_sequence_bit_for_bit(training):
    s = _stem()
    s.train(training)
    x = torch.randn(2, 3, 32, 32).requires_grad_(True)
    out, want = s(x), nn.Sequential.forward(s, x)
    assert type(out.grad_fn).__name__ != '_BnConvStemFnBackward'
    assert torch.equal(out, want)
    g, gw = torch.autograd.grad(out, [x] + list(s.parameters()), torch.ones_like(out)), torch.autograd.grad(want, [x] + list(s.parameters()), torch.ones_like(out))
    for u, v in zip(g, gw):
        assert torch.equal(u, v)
    assert not any('running' in k for k in s.state_dict())


class _Trajectory(nn.Module):
    """stands in for the ODE block: a trajectory of T fixed affine images of its input (no solve: the hand-off is what is tested)"""

    def __init__(self, t):
        super().__init__()
        self.t = t
        self.return_last_only = True

    def forward(self, x):
        if self.return_last_only:
            return x * (1.0 + 0.5 * (self.t - 1)) + 0.1 * (self.t - 1)
        return torch.stack([x * (1.0 + 0.5 * k) + 0.1 * k for k in range(self.t)])


def _ode2(t=3, c=64):
    import neural_ode_features_amd as nof
    ds = nof.ODEDownsample2(3, c, adjoint=True, norm='batch')
    ds.odeblock = _Trajectory(t)
    return ds


@pytest.mark.parametrize('apply_conv', [True, False])
@pytest.mark.parametrize('fused', [True, False])
def test_cpu_ode2_handoff_is_the_per_slice_modules_bit_for_bit(apply_conv, fused):
    ds = _ode2()
    ds.fused_handoff = fused
    assert isinstance(ds.norm[0], nn.BatchNorm2d) and not ds.norm[0].track_running_stats
    x = torch.randn(2, 3, 16, 16)
    last = ds.odeblock(ds.conv1(x))
    assert torch.equal(ds(x), ds.conv2(ds.norm(last.clone())))                       # model.py:223
    ds.odeblock.return_last_only = False
    ds.apply_conv = apply_conv
    traj = ds.odeblock(ds.conv1(x))
    normed = torch.stack([ds.norm(xi.clone()) for xi in traj])                       # model.py:214-216: slice by slice
    out, cont = ds(x)
    if apply_conv:
        want = torch.stack([ds.conv2(xi) for xi in normed])
        assert torch.equal(out, want) and torch.equal(cont, want[-1])
    else:
        assert torch.equal(out, normed) and torch.equal(cont, ds.conv2(normed[-1]))


# ---------------------------------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in K.ALL_CASES if c in K.SEEDS], ids=_id)
def test_seeds_of_the_gpu_cases_keep_every_relu_mask(case):
    """The seeds the GPU tests run their ordinary-parameter cases with: every ReLU mask of the fp32 CPU run agrees with the fp64
    run's, at a margin ratio no smaller than the yardstick's (bnconvstem_cases.py has the recipe)."""
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

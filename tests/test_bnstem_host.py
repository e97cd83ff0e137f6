"""Host side (no GPU) of the `norm='batch'` residual stem (stem.py `_BnStemFn`, csrc/bnstem_api.hip): the ABI, the launch plans of the
cases tests/test_gpu_bnstem.py runs (through node_bnstem_describe), the chunk policy and its switch, the argument checks of the C
ABI -- every one of which returns before a launch --, what the Python layer recognises and refuses, and the seeds."""
import ctypes as C
import os
import re

import pytest
import torch
from torch import nn

from tests import bnfunc_cases as B
from tests import bnstem_cases as S

NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED, NODE_ERR_WORKSPACE, NODE_ERR_ARG = -1, -2, -3, -4, -9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = 'NODE_TUNE_BNSTEM_MAXCHUNK'


def _id(case):
    cin, side, f, n = case
    return 'i%d_%s_f%d_n%d' % (cin, '%dx%d' % side if isinstance(side, tuple) else side, f, n)


def chunk_rows(rows, c, cap=128):
    """bnstem_chunk_rows of csrc/bnstem_api.hip, restated: at most `cap` chunks at C = 64, 2 cap / (C / 64) for wider tensors (never
    under 16), whole 32-row trips.  cap = 128 is bn_chunk_rows."""
    maxchunk = max(16, min(cap, 2 * cap // (c // 64)))
    cr = -(-rows // maxchunk)
    return max(32, (cr + 31) & ~31)


def tensors_of(case):
    """(rows, channels) of the four normalised tensors h0, h1, x1, h3"""
    n, _, h, w = S.shape_of(case)
    d = lambda s: (s - 1) // 2 + 1
    h0, w0 = h - 2, w - 2
    h1, w1 = d(h0), d(w0)
    return [(n * h0 * w0, 64), (n * h1 * w1, 64), (n * h1 * w1, 64), (n * d(h1) * d(w1), case[2])]


@pytest.fixture(autouse=True)
def _no_cap(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)


def test_exports_abi_version_and_layouts():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in ('node_bnstem_workspace_bytes', 'node_bnstem_describe', 'node_bnstem_fwd', 'node_bnstem_bwd'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additive
    header = open(os.path.join(ROOT, 'include', 'node_hip.h')).read()
    # the structures the four calls share with the GroupNorm stem and the batch-norm dynamics, field by field against the header
    m = re.search(r'typedef struct node_stem_shape \{(.*?)\} node_stem_shape;', header, re.S)
    assert re.findall(r'\b(n|in_ch|h|w|filters|eps)\b', m.group(1)) == [k for k, _ in _lib.NodeStemShape._fields_]
    assert C.sizeof(_lib.NodeStemShape) == 24
    m = re.search(r'typedef struct node_stem_params \{(.*?)\} node_stem_params;', header, re.S)
    assert tuple(re.findall(r'const float\* (\w+);', m.group(1))) == _lib.STEM_PARAM_FIELDS
    m = re.search(r'typedef struct node_stem_grads \{(.*?)\} node_stem_grads;', header, re.S)
    assert tuple(re.findall(r'float\* (\w+);', m.group(1))) == _lib.STEM_PARAM_FIELDS
    assert C.sizeof(_lib.NodeStemParams) == 16 * C.sizeof(C.c_void_p)
    m = re.search(r'typedef struct node_bnfunc_info \{(.*?)\} node_bnfunc_info;', header, re.S)
    assert [k.strip() for k in m.group(1).replace('int32_t', '').replace(';', '').split(',')] == [k for k, _ in _lib.NodeBnfuncInfo._fields_]
    assert C.sizeof(_lib.NodeBnfuncInfo) == 28
    for proto in ('size_t node_bnstem_workspace_bytes(const node_stem_shape* shape, int keep_for_backward);',
                  'int node_bnstem_describe(const node_stem_shape* shape, node_bnfunc_info out[4]);'):
        assert proto in header
    assert 'NODE_TUNE_STEM_W4 has no effect on this node' in header


def test_refused_and_taken_shapes():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    St = _lib.NodeStemShape
    size = lambda s, keep: lib.node_bnstem_workspace_bytes(C.byref(s), keep)
    info = (_lib.NodeBnfuncInfo * 4)()
    for bad, word, code in ((St(2, 4, 32, 32, 64, 1e-5), 'in_ch', NODE_ERR_UNSUPPORTED), (St(2, 3, 32, 32, 96, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED),
                            (St(2, 3, 32, 32, 32, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED), (St(2, 3, 32, 32, 8192, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED),
                            (St(2, 3, 4, 4, 64, 1e-5), 'shape', NODE_ERR_SHAPE), (St(2, 3, 64, 64, 64, 1e-5), '2400', NODE_ERR_UNSUPPORTED),
                            (St(1, 3, 5, 5, 64, 1e-5), 'more than one value per channel', NODE_ERR_UNSUPPORTED),
                            (St(20000, 3, 50, 50, 64, 1e-5), '2^31', NODE_ERR_UNSUPPORTED), (St(0, 3, 32, 32, 64, 1e-5), 'shape', NODE_ERR_SHAPE)):
        for keep in (0, 1):
            assert size(bad, keep) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_bnstem_fwd(C.byref(bad), None, None, None, 1, None, 0, None) == code
        assert lib.node_bnstem_bwd(C.byref(bad), None, None, None, None, None, None, 0, None) == code
        assert lib.node_bnstem_describe(C.byref(bad), info) == code
    assert size(St(2, 3, 5, 5, 64, 1e-5), 1) > 0                         # two values per channel at the last norm
    assert size(St(128, 3, 32, 32, 256, 1e-5), 1) < (1 << 30)
    for filters in (192, 384):                                           # BatchNorm has no groups: what the GroupNorm stem refuses
        assert lib.node_stem_workspace_bytes(C.byref(St(2, 3, 32, 32, filters, 1e-5))) == 0
        assert size(St(2, 3, 32, 32, filters, 1e-5), 1) > 0
    assert lib.node_bnstem_workspace_bytes(None, 1) == 0
    assert lib.node_bnstem_describe(C.byref(St(2, 3, 32, 32, 64, 1e-5)), None) == NODE_ERR_NULL
    assert lib.node_bnstem_describe(None, info) == NODE_ERR_NULL


@pytest.mark.parametrize('case', S.ALL_CASES, ids=_id)
def test_every_case_has_a_workspace_and_the_plan_of_the_chunk_function(case):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    n, cin, h, w = S.shape_of(case)
    s = _lib.NodeStemShape(n, cin, h, w, case[2], 1e-5)
    keep, scratch = lib.node_bnstem_workspace_bytes(C.byref(s), 1), lib.node_bnstem_workspace_bytes(C.byref(s), 0)
    assert 0 < scratch < keep
    plan = _lib.bnstem_plan(n, cin, h, w, case[2])
    assert len(plan) == 4
    for d, (rows, c) in zip(plan, tensors_of(case)):
        cr = chunk_rows(rows, c)
        nchunk = -(-rows // cr)
        assert (d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows'], d['column_tiles']) == (rows, cr, nchunk, rows - (nchunk - 1) * cr, c // 64), (case, d)
        assert d['wgrad_nsplit'] >= 1 and d['wgrad_rows_per_split'] % 16 == 0
    # at the default cap the policy IS the one of the other batch-norm nodes (bn_chunk_rows, through the trunk's describe call)
    dn = lambda v: (v - 1) // 2 + 1
    h0, w0 = h - 2, w - 2
    sizes = [(h0, w0), (dn(h0), dn(w0)), (dn(h0), dn(w0)), (dn(dn(h0)), dn(dn(w0)))]
    for d, (hh, ww), (rows, c) in zip(plan, sizes, tensors_of(case)):
        t = _lib.describe_bntrunk(n, c, hh, ww, 1)
        assert (t['rows'], t['chunk_rows'], t['nchunk'], t['last_chunk_rows']) == (d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows'])


def test_small_cases_run_one_trip():
    from neural_ode_features_amd import _lib
    for case in S.CASES:
        n, cin, h, w = S.shape_of(case)
        for d in _lib.bnstem_plan(n, cin, h, w, case[2]):
            assert d['chunk_rows'] == 32 and d['nchunk'] == -(-d['rows'] // 32), (case, d)
    assert _lib.bnstem_plan(4, 1, 6, 5, 64)[3]['rows'] == 4


@pytest.mark.parametrize('case', list(S.MULTI_CASES), ids=_id)
def test_multi_chunk_cases_reach_their_regimes(case):
    """A later change of the chunk or split heuristics cannot quietly empty these cases."""
    from neural_ode_features_amd import _lib
    n, cin, h, w = S.shape_of(case)
    plan = _lib.bnstem_plan(n, cin, h, w, case[2])
    for norm, regime in S.MULTI_CASES[case]:
        assert S.REGIMES[regime](plan[norm]), (case, norm, regime, plan[norm])
    want = {(3, 32, 64, 5): [(4500, 64, 71, 20), (1125, 32, 36, 5)], (3, 32, 64, 33): [(29700, 256, 117, 4), (7425, 64, 117, 1)]}[case]
    assert [(d['rows'], d['chunk_rows'], d['nchunk'], d['last_chunk_rows']) for d in plan[:2]] == want


def test_the_chunk_cap_changes_describe_and_nothing_else(monkeypatch):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    case = (3, 32, 64, 33)
    n, cin, h, w = S.shape_of(case)
    s = _lib.NodeStemShape(n, cin, h, w, case[2], 1e-5)
    default = _lib.bnstem_plan(n, cin, h, w, case[2])
    trunk = _lib.describe_bntrunk(33, 64, 8, 8)
    func = _lib.describe_bnfunc(84, 64, 7, 7)
    for unset in ('0', '128', ''):
        monkeypatch.setenv(ENV, unset)
        assert _lib.bnstem_plan(n, cin, h, w, case[2]) == default
    monkeypatch.setenv(ENV, '1024')
    fine = _lib.bnstem_plan(n, cin, h, w, case[2])
    assert fine != default
    for d, (rows, c) in zip(fine, tensors_of(case)):
        cr = chunk_rows(rows, c, 1024)
        assert (d['chunk_rows'], d['nchunk']) == (cr, -(-rows // cr))
    assert fine[0]['chunk_rows'] == 32 and fine[0]['nchunk'] == 929
    # the convolutions' split-K plans, the other batch-norm nodes and the GroupNorm stem do not read it
    for a, b in zip(fine, default):
        assert (a['rows'], a['column_tiles'], a['wgrad_nsplit'], a['wgrad_rows_per_split']) == (b['rows'], b['column_tiles'], b['wgrad_nsplit'], b['wgrad_rows_per_split'])
    assert _lib.describe_bntrunk(33, 64, 8, 8) == trunk and _lib.describe_bnfunc(84, 64, 7, 7) == func
    assert lib.node_bnstem_workspace_bytes(C.byref(s), 1) > 0
    # NODE_TUNE_STEM_W4 has no effect on this node
    monkeypatch.delenv(ENV)
    monkeypatch.setenv('NODE_TUNE_STEM_W4', '0')
    s8 = _lib.NodeStemShape(8, 3, 32, 32, 128, 1e-5)
    off = lib.node_bnstem_workspace_bytes(C.byref(s8), 1)
    monkeypatch.setenv('NODE_TUNE_STEM_W4', '1')
    assert lib.node_bnstem_workspace_bytes(C.byref(s8), 1) == off and _lib.bnstem_plan(8, 3, 32, 32, 128) == _lib.bnstem_plan(8, 3, 32, 32, 128)


def test_null_misaligned_and_short_workspace_arguments_are_rejected_before_any_launch():
    """Every call below returns before its first launch (this test runs without a GPU); the pointers are host memory that is
    never read."""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeStemShape(2, 3, 32, 32, 64, 1e-5)
    s = C.byref(shape)
    nbytes = lib.node_bnstem_workspace_bytes(s, 1)
    buf = (C.c_char * 16384)()
    base = (C.addressof(buf) + 255) & ~255
    P = _lib.NodeStemParams

    def tensors(hole=None, odd=None):
        vals = [base + 256 * k for k in range(16)]
        if hole is not None:
            vals[hole] = None
        if odd is not None:
            vals[odd] += 4
        return C.byref(P(*vals))
    good = tensors()
    x, out, ws = base + 4352, base + 4608, base + 4864
    fwd, bwd = lib.node_bnstem_fwd, lib.node_bnstem_bwd
    assert fwd(None, good, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, None, x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, tensors(hole=13), x, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, tensors(odd=2), x, out, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, None, out, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x + 4, out, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out + 8, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out, 1, None, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, out, 1, ws + 16, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out, 1, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    assert 'too small' in lib.node_last_error().decode()
    assert fwd(s, good, x, out, 0, ws, lib.node_bnstem_workspace_bytes(s, 0) - 1, None) == NODE_ERR_WORKSPACE
    assert bwd(None, good, x, out, good, x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, None, x, out, good, x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, tensors(hole=0), x, out, good, x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, None, out, good, x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, None, good, x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, out + 4, good, x, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, out, None, None, ws, nbytes, None) == NODE_ERR_NULL              # neither grads nor d_x: nothing to compute
    assert bwd(s, good, x, out, tensors(hole=5), x, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, out, tensors(odd=15), None, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, out, None, x + 8, ws, nbytes, None) == NODE_ERR_ARG
    for grads, d_x in ((good, x), (good, None), (None, x)):                                  # each of the three ways to ask
        assert bwd(s, good, x, out, grads, d_x, None, nbytes, None) == NODE_ERR_NULL
        assert bwd(s, good, x, out, grads, d_x, ws + 16, nbytes, None) == NODE_ERR_ARG
        assert bwd(s, good, x, out, grads, d_x, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------------------------
# recognition, the CPU path
# ---------------------------------------------------------------------------------------------------------------------
def _stem(filters=64, in_ch=3, norm='batch'):
    import neural_ode_features_amd as nof
    return nof.ODENet(in_ch, out=10, n_filters=filters, downsample='residual', adjoint=True, norm=norm).downsample.module


def test_recognition_of_stems():
    from neural_ode_features_amd import stem
    s = _stem(128)
    ps = stem._bn_params_of(s)
    assert ps is not None and len(ps) == 16
    assert [tuple(p.shape) for p in ps] == [(64, 3, 3, 3), (64,), (64,), (64,), (64, 64, 3, 3), (64,), (64,), (64, 64, 3, 3), (64, 64, 1, 1),
                                            (64,), (64,), (128, 64, 3, 3), (128,), (128,), (128, 128, 3, 3), (128, 64, 1, 1)]
    assert {id(p) for p in ps} == {id(p) for p in s.parameters()} and ps[4] is s[1].conv1.weight and ps[8] is s[1].downsample.weight
    assert stem._params_of(s) is None                                              # GroupNorm only, as it was
    gn = _stem(norm='group')
    assert len(stem._params_of(gn)) == 16 and stem._bn_params_of(gn) is None
    assert stem.ResidualStem.fused_batch is True
    # running statistics, no affine parameters, another eps in one slot, a GroupNorm in one slot: the module sequence
    tracked = _stem()
    tracked[2].norm1 = nn.BatchNorm2d(64)
    assert stem._bn_params_of(tracked) is None
    plain = _stem()
    plain[1].norm2 = nn.BatchNorm2d(64, affine=False, track_running_stats=False)
    assert stem._bn_params_of(plain) is None
    eps = _stem()
    eps[2].norm2.eps = 1e-3
    assert stem._bn_params_of(eps) is None
    mixed = _stem()
    mixed[1].norm1 = nn.GroupNorm(32, 64)
    assert stem._bn_params_of(mixed) is None and stem._params_of(mixed) is None
    wrong = _stem()
    wrong[1].conv1 = nn.Conv2d(64, 64, 3, 1, 1, bias=False)                          # the geometry checks of _params_of
    assert stem._bn_params_of(wrong) is None
    # filters = 96 is recognised as a stem and refused by shape (bn_fusable needs a HIP tensor: a CPU tensor is refused first)
    assert stem._bn_params_of(_stem(96)) is not None
    assert not stem.bn_fusable(s, torch.randn(2, 3, 32, 32))
    # hooks on a sub-module send the stem to the modules; a hook on the stem itself does not
    hooked = _stem()
    handle = hooked[1].norm1.register_forward_hook(lambda m, i, o: None)
    assert stem._hooked(hooked)
    handle.remove()
    handle = hooked.register_forward_hook(lambda m, i, o: None)
    assert not stem._hooked(hooked)
    handle.remove()


@pytest.mark.parametrize('training', [True, False])
def test_cpu_path_is_the_module_sequence_bit_for_bit(training):
    s = _stem()
    s.train(training)
    x = torch.randn(2, 3, 32, 32).requires_grad_(True)
    out, want = s(x), nn.Sequential.forward(s, x)
    assert type(out.grad_fn).__name__ != '_BnStemFnBackward'
    assert torch.equal(out, want)
    g, gw = torch.autograd.grad(out, [x] + list(s.parameters()), torch.ones_like(out)), torch.autograd.grad(want, [x] + list(s.parameters()), torch.ones_like(out))
    for u, v in zip(g, gw):
        assert torch.equal(u, v)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        s(torch.randn(1, 3, 5, 5))


def test_train_and_eval_agree_without_running_statistics():
    s = _stem()
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        a = s.train()(x)
        b = s.eval()(x)
    assert torch.equal(a, b)
    assert not any('running' in k for k in s.state_dict())


# ---------------------------------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in S.ALL_CASES if c in S.SEEDS], ids=_id)
def test_seeds_of_the_gpu_cases_keep_every_relu_mask(case):
    """The seeds tests/test_gpu_bnstem.py runs its ordinary-parameter cases with: every ReLU mask of the fp32 CPU run agrees with
    the fp64 run's, at a margin ratio no smaller than the yardstick's (bnstem_cases.py has the recipe)."""
    agree, margin, ratio = S.margin_ratio(case, S.SEEDS[case])
    assert agree and margin > 0
    assert ratio >= B.margin_ratio(*B.RATIO_YARDSTICK)[2], (case, ratio)


@pytest.mark.parametrize('mode', ['kinkfree', 'split'])
@pytest.mark.parametrize('case', S.ALL_CASES, ids=_id)
def test_kinkfree_and_split_sets_have_no_kink(case, mode):
    constant, margin = S.sign_condition(case, mode)
    assert constant and margin > 0.5, (case, mode, margin)


def test_every_case_runs_something():
    assert [c for c in S.ALL_CASES if c not in S.SEEDS] == [(3, 32, 64, 33)]       # every other case runs 'ordinary' too
    for case in S.ALL_CASES:
        modes = [m for _, m in S.runs(case)]
        assert 'kinkfree' in modes and 'split' in modes and (('ordinary' in modes) == (case in S.SEEDS))

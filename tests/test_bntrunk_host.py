"""Host side (no GPU) of the `norm='batch'` residual trunk and classifier head (resnet.py `_BnTrunkFn`, head.py `bn_head_pool`,
csrc/bntrunk_api.hip, csrc/bnhead_api.hip): the launch regimes of the cases tests/test_gpu_bntrunk.py runs (through
node_bntrunk_describe), their seeds, what the Python layer recognises and refuses, and the argument checks of the C ABI, every one
of which returns before a launch."""
import ctypes as C

import pytest
import torch
from torch import nn

from tests import bnfunc_cases as B
from tests import bnhead_cases as H
from tests import bntrunk_cases as T

NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED, NODE_ERR_WORKSPACE, NODE_ERR_ARG = -1, -2, -3, -4, -9


def _id(case):
    c, side, n, blocks = case
    return 'c%d_%s_n%d_b%d' % (c, '%dx%d' % side if isinstance(side, tuple) else side, n, blocks)


def test_exports_and_abi_version():
    from neural_ode_features_amd import _lib
    for name in ('node_bntrunk_workspace_bytes', 'node_bntrunk_fwd', 'node_bntrunk_bwd', 'node_bntrunk_describe',
                 'node_bnhead_scratch_bytes', 'node_bnhead_fwd', 'node_bnhead_bwd'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.load().node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additive


@pytest.mark.parametrize('case', T.ALL_CASES, ids=_id)
def test_every_case_has_a_workspace(case):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    n, c, h, w = T.shape_of(case)
    s = _lib.NodeTrunkShape(n, c, h, w, case[3], 1e-5)
    keep, scratch = lib.node_bntrunk_workspace_bytes(C.byref(s), 1), lib.node_bntrunk_workspace_bytes(C.byref(s), 0)
    assert 0 < scratch < keep


def test_refused_shapes():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    S = _lib.NodeTrunkShape
    size = lambda s, keep: lib.node_bntrunk_workspace_bytes(C.byref(s), keep)
    assert size(S(128, 256, 8, 8, 6, 1e-5), 1) < (4 << 30)
    for bad, word, code in ((S(2, 96, 8, 8, 6, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED), (S(2, 64, 8, 8, 0, 1e-5), 'blocks', NODE_ERR_UNSUPPORTED),
                            (S(2, 32, 8, 8, 6, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED), (S(2, 8192, 8, 8, 6, 1e-5), 'multiple of 64', NODE_ERR_UNSUPPORTED),
                            (S(8192, 4096, 8, 8, 6, 1e-5), '2^31', NODE_ERR_UNSUPPORTED), (S(0, 64, 8, 8, 6, 1e-5), 'shape', NODE_ERR_SHAPE),
                            (S(2, 64, 0, 8, 6, 1e-5), 'shape', NODE_ERR_SHAPE)):
        for keep in (0, 1):
            assert size(bad, keep) == 0, bad
        assert word in lib.node_last_error().decode(), (word, lib.node_last_error())
        assert lib.node_bntrunk_fwd(C.byref(bad), None, None, None, None, 1, None, 0, None) == code
        assert lib.node_bntrunk_describe(C.byref(bad), C.byref(_lib.NodeBnfuncInfo())) == code
    assert size(S(2, 64, 1, 1, 1, 1e-5), 1) > 0              # no time channel, no border classes: h w >= 1 is enough
    assert lib.node_bntrunk_workspace_bytes(None, 1) == 0
    assert lib.node_bntrunk_describe(C.byref(S(2, 64, 8, 8, 1, 1e-5)), None) == NODE_ERR_NULL
    H = _lib.NodeBnfuncShape
    assert lib.node_bnhead_scratch_bytes(C.byref(H(128, 256, 8, 8, 1e-5))) > 0
    for bad in (H(2, 96, 8, 8, 1e-5), H(2, 16, 8, 8, 1e-5), H(0, 64, 8, 8, 1e-5)):
        assert lib.node_bnhead_scratch_bytes(C.byref(bad)) == 0
    assert lib.node_bnhead_scratch_bytes(None) == 0


def test_null_misaligned_and_short_workspace_arguments_are_rejected_before_any_launch():
    """Every call below returns before its first launch (this test runs without a GPU); the pointers are host memory that is
    never read."""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeTrunkShape(2, 64, 8, 8, 2, 1e-5)
    s = C.byref(shape)
    nbytes = lib.node_bntrunk_workspace_bytes(s, 1)
    buf = (C.c_char * 16384)()
    base = (C.addressof(buf) + 255) & ~255
    Blk = _lib.NodeTrunkBlock

    def blocks(hole=None, odd=None):
        arr = (Blk * 2)()
        for i in range(2):
            vals = [base + 256 * (6 * i + k) for k in range(6)]
            if hole == (i, 0):
                vals[4] = None
            if odd == i:
                vals[2] += 4
            arr[i] = Blk(*vals)
        return arr
    good, holed, odd = blocks(), blocks(hole=(1, 0)), blocks(odd=1)
    x, out, ws = base + 4096, base + 4352, base + 4608
    fwd, bwd = lib.node_bntrunk_fwd, lib.node_bntrunk_bwd
    assert fwd(None, good, x, out, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, None, x, out, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, holed, x, out, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, odd, x, out, None, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, None, out, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, None, None, 1, ws, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x + 4, out, None, 1, ws, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out, out + 8, 1, ws, nbytes, None) == NODE_ERR_ARG          # taps are optional, but aligned when given
    assert fwd(s, good, x, out, None, 1, None, nbytes, None) == NODE_ERR_NULL
    assert fwd(s, good, x, out, None, 1, ws + 16, nbytes, None) == NODE_ERR_ARG
    assert fwd(s, good, x, out, None, 1, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    assert 'too small' in lib.node_last_error().decode()
    assert fwd(s, good, x, out, None, 0, ws, lib.node_bntrunk_workspace_bytes(s, 0) - 1, None) == NODE_ERR_WORKSPACE
    assert bwd(None, good, x, good, out, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, None, x, good, out, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, None, good, out, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, None, out, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, holed, out, ws, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, odd, out, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, good, None, ws, nbytes, None) == NODE_ERR_NULL             # d_x is required: the stem trains behind the trunk
    assert bwd(s, good, x, good, out + 8, ws, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, good, out, None, nbytes, None) == NODE_ERR_NULL
    assert bwd(s, good, x, good, out, ws + 16, nbytes, None) == NODE_ERR_ARG
    assert bwd(s, good, x, good, out, ws, nbytes - 1, None) == NODE_ERR_WORKSPACE
    # the head
    hs = C.byref(_lib.NodeBnfuncShape(2, 64, 8, 8, 1e-5))
    p = [base + 256 * i for i in range(12)]
    hf, hb = lib.node_bnhead_fwd, lib.node_bnhead_bwd
    assert hf(None, p[0], p[1], p[2], None, p[3], p[4], p[5], None) == NODE_ERR_NULL
    for k in (0, 1, 2, 4, 5, 6):          # z, gamma, beta, pooled, stats, scratch (scale is optional)
        args = [p[0], p[1], p[2], None, p[3], p[4], p[5]]
        args[k] = None
        assert hf(hs, *args, None) == NODE_ERR_NULL, k
    assert hf(hs, p[0] + 2, p[1], p[2], None, p[3], p[4], p[5], None) == NODE_ERR_ARG
    assert hf(hs, p[0], p[1], p[2], None, p[3], p[4], p[5] + 4, None) == NODE_ERR_ARG
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        args = [p[0], p[1], p[2], None, p[3], p[4], p[5], p[6], p[7], p[8]]
        args[k] = None
        assert hb(hs, *args, None) == NODE_ERR_NULL, k
    assert hb(hs, p[0], p[1], p[2], None, p[3], p[4], p[5], p[6], p[7], p[8] + 4, None) == NODE_ERR_ARG
    assert hb(C.byref(_lib.NodeBnfuncShape(2, 96, 8, 8, 1e-5)), p[0], p[1], p[2], None, p[3], p[4], p[5], p[6], p[7], p[8], None) == NODE_ERR_UNSUPPORTED


@pytest.mark.parametrize('case', list(T.MULTI_CASES), ids=_id)
def test_multi_row_cases_reach_their_regimes(case):
    """The chunks come from the same bn_chunk_rows as the dynamics': the regimes of bnfunc_cases.MULTI_CASES carry over, and a later
    change of the chunk or split heuristics cannot quietly empty these cases."""
    from neural_ode_features_amd import _lib
    n, c, h, w = T.shape_of(case)
    d = _lib.describe_bntrunk(n, c, h, w, case[3])
    assert d == _lib.describe_bnfunc(n, c, h, w)
    for regime in T.MULTI_CASES[case]:
        assert B.REGIMES[regime](d), (case, regime, d)
    assert d['rows'] == n * h * w and d['column_tiles'] == c // 64


def test_small_cases_run_one_trip_and_1x1_is_described():
    from neural_ode_features_amd import _lib
    for case in T.CASES:
        n, c, h, w = T.shape_of(case)
        d = _lib.describe_bntrunk(n, c, h, w, case[3])
        assert d['chunk_rows'] == 32 and d['nchunk'] == -(-n * h * w // 32), (case, d)
    assert _lib.describe_bntrunk(4, 64, 1, 1, 1)['last_chunk_rows'] == 4


@pytest.mark.parametrize('case', [c for c in T.ALL_CASES if c in T.SEEDS], ids=_id)
def test_seeds_of_the_gpu_cases_keep_every_relu_mask(case):
    """The seeds tests/test_gpu_bntrunk.py runs its ordinary-parameter cases with: every ReLU mask of the fp32 CPU run agrees with
    the fp64 run's, at a margin ratio no smaller than the yardstick's (bntrunk_cases.py has the recipe)."""
    agree, margin, ratio = T.margin_ratio(case, T.SEEDS[case])
    assert agree and margin > 0
    assert ratio >= B.margin_ratio(*B.RATIO_YARDSTICK)[2], (case, ratio)


@pytest.mark.parametrize('mode', ['kinkfree', 'split'])
@pytest.mark.parametrize('case', [(64, 7, 3, 2), (128, 8, 2, 6), (64, 7, 84, 2)], ids=_id)
def test_kinkfree_and_split_sets_have_no_kink(case, mode):
    constant, margin = T.sign_condition(case, mode)
    assert constant and margin > 1.0, (case, mode, margin)


def test_every_case_runs_something():
    for case in T.ALL_CASES:
        modes = [m for _, m in T.runs(case)]
        assert 'kinkfree' in modes and 'split' in modes and (('ordinary' in modes) == (case in T.SEEDS))


def _trunk(c=64, blocks=2, norm='batch'):
    import neural_ode_features_amd as nof
    return nof.resnet.ResidualTrunk(c, blocks, norm=norm)


def test_recognition_of_trunks():
    from neural_ode_features_amd import resnet
    t = _trunk()
    form, ps = resnet._form_of(t)
    assert form == 'batch' and len(ps) == 12 and resnet._params_of(t) is not None
    assert [tuple(p.shape) for p in ps[:6]] == [(64,), (64,), (64, 64, 3, 3), (64,), (64,), (64, 64, 3, 3)]
    assert resnet._form_of(_trunk(norm='group'))[0] == 'group'
    assert resnet.ResidualTrunk.fused_batch is True
    # running statistics, no affine parameters, another eps in one block, mixed norms, hooks: the module sequence
    tracked = _trunk()
    tracked[1].norm2 = nn.BatchNorm2d(64)
    assert resnet._params_of(tracked) is None
    plain = _trunk()
    plain[0].norm1 = nn.BatchNorm2d(64, affine=False, track_running_stats=False)
    assert resnet._params_of(plain) is None
    eps = _trunk()
    eps[1].norm1.eps = 1e-3
    assert resnet._params_of(eps) is None
    mixed = _trunk()
    mixed[1].norm1 = nn.GroupNorm(32, 64)
    assert resnet._params_of(mixed) is None
    hooked = _trunk()
    handle = hooked[0].register_forward_hook(lambda m, i, o: None)
    assert resnet._params_of(hooked) is None
    handle.remove()
    assert resnet._params_of(hooked) is not None
    # C = 96 is recognised as a trunk and refused by shape (fusable needs a HIP tensor: a CPU tensor is refused first)
    assert resnet._form_of(_trunk(96))[0] == 'batch'
    x = torch.randn(2, 64, 8, 8)
    assert not resnet.fusable(t, x)
    out = t(x.requires_grad_(True))
    assert type(out.grad_fn).__name__ != '_BnTrunkFnBackward'
    taps = t.forward_taps(x)[1]
    assert len(taps) == 2 and torch.equal(taps[-1], out)


def test_recognition_of_heads():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import head
    assert nof.FCClassifier.fused_batch is True
    clf = nof.FCClassifier(64, norm='batch')
    bn = clf.module[0]
    assert isinstance(bn, nn.BatchNorm2d) and not bn.track_running_stats

    class Dev:          # what bn_head_fusable asks of a tensor, without a device
        is_cuda, dtype, shape = True, torch.float32, (2, 64, 8, 8)

        def dim(self):
            return 4
    x = torch.randn(2, 64, 8, 8)
    assert not head.bn_head_fusable(x, bn)                                       # a CPU tensor
    assert not clf._batch_head(x, bn)
    assert not head.bn_head_fusable(x, nn.BatchNorm2d(64))                       # running statistics
    assert not head.bn_head_fusable(x, nn.BatchNorm2d(64, affine=False, track_running_stats=False))
    assert not head.bn_head_fusable(x, nn.GroupNorm(32, 64))
    # the CPU path is the module sequence, dropout and feature extraction included
    out = clf(x)
    assert out.shape == (2, 10) and torch.equal(out, clf.module(x))
    # N H W = 1: nn.BatchNorm2d refuses it (with batch statistics, in training and evaluation alike)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        clf(torch.randn(1, 64, 1, 1))
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        _trunk()(torch.randn(1, 64, 1, 1))


@pytest.mark.parametrize('case', H.CASES + [H.OFFSET_CASE], ids=lambda c: 'n%d_c%d_%dx%d' % c)
def test_seeds_of_the_head_cases_keep_the_relu_mask(case):
    agree, margin, ratio = H.margin_ratio(case, H.SEEDS[case])
    assert agree and margin > 0 and ratio >= B.margin_ratio(*B.RATIO_YARDSTICK)[2], (case, margin, ratio)
    for mode in ('kinkfree', 'split'):
        bn, ref = H.norm_pair(case, H.KINK_FREE_SEED, mode)
        with torch.no_grad():
            assert float(ref(H.case_inputs(case, H.KINK_FREE_SEED)[0].double()).abs().min()) > 1.0

"""No GPU: the banded residual stem's probes (node_stem_banded_workspace_bytes / node_stem_banded_describe), the Python gate
`stem.banded_fusable`, and the seed rule of tests/stem_banded_cases.py on the two CPU runs."""
import ctypes as C

import pytest
import torch

from tests import stem_banded_cases as B

NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED = -1, -2, -3
ENTRIES = ('node_stem_banded_workspace_bytes', 'node_stem_banded_describe', 'node_stem_banded_fwd', 'node_stem_banded_bwd',
           'node_stem_banded_bwd_dx')


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv('NODE_TUNE_STEM_BANDED', raising=False)
    monkeypatch.delenv('NODE_TUNE_STEM_BAND_PX', raising=False)
    monkeypatch.delenv('NODE_TUNE_STEM_W4', raising=False)


def test_entries_are_exported_and_bound():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additions only
    # node_stem_gn_info + five int32_t; four of those + 1 + 4 + 4 int32_t
    assert C.sizeof(_lib.NodeStemBandedGnInfo) == 24 + 20 and C.sizeof(_lib.NodeStemBandedInfo) == 4 * 44 + 4 + 16 + 16


def test_accepted_shapes_have_a_workspace():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    assert [(n, c, h, w, f) for n, c, h, w, f in B.SHAPES.values()][:6] == [
        (1, 3, 51, 51, 64), (2, 3, 64, 64, 128), (2, 3, 64, 64, 1024), (3, 1, 53, 70, 64), (1, 3, 102, 102, 64), (2, 3, 32, 32, 256)]
    for n, c, h, w, f in B.SHAPES.values():
        sh = _lib.NodeStemShape(n, c, h, w, f, 1e-5)
        nbytes = lib.node_stem_banded_workspace_bytes(C.byref(sh))
        assert nbytes > 0, (n, c, h, w, f)
        # the band partials lie behind the resident plan's pieces: never less than the resident node asks for
        resident = lib.node_stem_workspace_bytes(C.byref(sh))
        assert resident == 0 or nbytes >= resident
    # shapes the resident node takes keep the resident plan: nothing banded, nothing added
    sh = _lib.NodeStemShape(2, 3, 32, 32, 256, 1e-5)
    assert lib.node_stem_banded_workspace_bytes(C.byref(sh)) == lib.node_stem_workspace_bytes(C.byref(sh))


def test_refusals_return_the_codes_of_the_resident_probe_and_zero_the_record():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    St = _lib.NodeStemShape
    info = _lib.NodeStemBandedInfo()
    assert lib.node_stem_banded_describe(None, C.byref(info)) == NODE_ERR_NULL
    assert lib.node_stem_banded_describe(C.byref(St(2, 3, 64, 64, 64, 1e-5)), None) == NODE_ERR_NULL
    # R2 F = 8192 x 64 x 4096 = 2^31 while n H0 W0 64 = 8192 x 1024 x 64 = 2^29
    big = St(8192, 3, 34, 34, 4096, 1e-5)
    assert 8192 * 8 * 8 * 4096 == 2 ** 31 and 8192 * 32 * 32 * 64 < 2 ** 31
    for bad, code in ((St(0, 3, 64, 64, 64, 1e-5), NODE_ERR_SHAPE), (St(2, 3, 5, 4, 64, 1e-5), NODE_ERR_SHAPE),
                      (St(2, 4, 64, 64, 64, 1e-5), NODE_ERR_UNSUPPORTED), (St(2, 3, 64, 64, 24, 1e-5), NODE_ERR_UNSUPPORTED),
                      (St(2, 3, 64, 64, 192, 1e-5), NODE_ERR_UNSUPPORTED), (big, NODE_ERR_UNSUPPORTED)):
        info.takes_w4 = 7
        info.gn[0].banded = 7
        assert lib.node_stem_banded_describe(C.byref(bad), C.byref(info)) == code and len(lib.node_last_error()) > 0
        assert bytes(info) == bytes(C.sizeof(info))                       # zeroed
        assert lib.node_stem_banded_workspace_bytes(C.byref(bad)) == 0
        small = St(bad.n, bad.in_ch, min(bad.h, 32), min(bad.w, 32), bad.filters, 1e-5)
        if bad is not big:                                                # the same defect, the same code from the resident probe
            assert lib.node_stem_describe(C.byref(small), C.byref(_lib.NodeStemInfo())) == code
    # one step below the limit is taken
    assert lib.node_stem_banded_workspace_bytes(C.byref(St(8191, 3, 34, 34, 4096, 1e-5))) > 0


def test_describe_reports_which_norms_are_banded(monkeypatch):
    from neural_ode_features_amd import _lib
    banded = lambda d: [g['banded'] for g in d['gn']]
    d = _lib.stem_banded_plan(1, 3, 51, 51, 64)
    assert banded(d) == [True, False, False, False]
    g = d['gn'][0]
    assert (g['hw'], g['channels'], g['cpg'], g['cb'], g['blocks_per_sample']) == (2401, 64, 2, 64, 1)
    assert g['band_px'] == 128 and g['bands_per_sample'] == 19 and g['grid'] == g['grid_first'] == g['grid_second'] == 19
    r = d['gn'][1]                                                        # resident: the record of the launch stem_gn_cb plans
    assert (r['hw'], r['cb'], r['grid'], r['band_px'], r['bands_per_sample'], r['grid_first'], r['grid_second']) == (625, 16, 4, 0, 0, 0, 0)
    assert banded(_lib.stem_banded_plan(1, 3, 102, 102, 64)) == [True, True, True, False]
    d64 = _lib.stem_banded_plan(2, 3, 64, 64, 1024)
    assert banded(d64) == [True, False, False, False] and not d64['takes_w4']
    assert d64['gn'][0]['bands_per_sample'] == -(-3844 // 128) and d64['gn'][0]['grid'] == 2 * 31
    assert d64['gn'][3]['cpg'] == 32 and d64['gn'][3]['cb'] == 64        # (resident: 256 px x 64 channels)
    d32 = _lib.stem_banded_plan(2, 3, 32, 32, 256)
    assert banded(d32) == [False] * 4
    res = _lib.stem_plan(2, 3, 32, 32, 256)
    assert [{k: g[k] for k in res['gn'][0]} for g in d32['gn']] == res['gn'] and d32['wgrad'] == res['wgrad']
    monkeypatch.setenv('NODE_TUNE_STEM_BANDED', 'all')
    d32 = _lib.stem_banded_plan(2, 3, 32, 32, 256)
    assert banded(d32) == [True] * 4 and [g['cb'] for g in d32['gn']] == [64] * 4
    assert [g['blocks_per_sample'] for g in d32['gn']] == [1, 1, 1, 4]
    assert _lib.stem_plan(2, 3, 32, 32, 256) == res                       # the resident node does not read the switch
    # F(4x4,3x3) follows stem_takes_w4 unchanged: the fourth norm then runs inside that pipeline, never banded
    d8 = _lib.stem_banded_plan(8, 3, 32, 32, 256)
    assert d8['takes_w4'] and banded(d8) == [True, True, True, False]
    monkeypatch.setenv('NODE_TUNE_STEM_BAND_PX', '16')
    for n, c, h, w, f in B.SHAPES.values():
        for g in _lib.stem_banded_plan(n, c, h, w, f)['gn']:
            assert g['banded'] and g['band_px'] == 16 and g['bands_per_sample'] == -(-g['hw'] // 16)
            assert g['grid'] == n * g['bands_per_sample'] * g['blocks_per_sample']
    monkeypatch.delenv('NODE_TUNE_STEM_BANDED')
    assert _lib.stem_banded_plan(1, 3, 51, 51, 64)['gn'][0]['bands_per_sample'] == -(-2401 // 16)


def test_banded_fusable_on_what_the_cpu_can_tell():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import stem as S
    stem = nof.ODENet(3, out=10, n_filters=64, downsample='residual', adjoint=True).downsample.module
    assert isinstance(stem, S.ResidualStem) and S.ResidualStem.fused_banded in (True, False)
    x = torch.randn(2, 3, 64, 64)
    assert not S.banded_fusable(stem, x)                                  # a CPU tensor
    assert not S.banded_fusable(stem, x.double()) and not S.banded_fusable(stem, None)
    assert not S.banded_fusable(stem, x.requires_grad_(True), input_grad=False)
    # the gate's device-independent conditions, on a stand-in whose tensors claim to be on a HIP device
    class OnDevice(torch.Tensor):
        is_cuda = True

    def fake(t):
        return t.as_subclass(OnDevice)
    # (parameters stay on the CPU: the gate must refuse them whatever the input claims)
    assert not S.banded_fusable(stem, fake(torch.randn(2, 3, 64, 64)))
    hooked = nof.ODENet(3, out=10, n_filters=64, downsample='residual', adjoint=True).downsample.module
    handle = hooked[1].conv1.register_forward_hook(lambda m, i, o: None)
    assert S._hooked(hooked) and not S._hooked(stem)
    handle.remove()
    assert not S._hooked(hooked)
    # a CPU batch of 64-pixel images runs the module sequence
    out = stem(torch.randn(1, 3, 64, 64))
    assert out.shape == (1, 64, 16, 16) and 'Stem' not in type(out.grad_fn).__name__


@pytest.mark.parametrize('name', [k for k in B.SHAPES if k not in B.RELATIVE_L2])
def test_the_recorded_seed_meets_the_seed_rule(name):
    """No GroupNorm output of the float64 run within 8 x the float32 CPU run's distance of zero (both runs on the CPU, forward only)."""
    assert isinstance(B.SEEDS[name], int) and B.SEEDS[name] >= 1
    margin = B.seed_margin(name)
    print('%s: seed %d, min |u| / (8 x fp32 distance) = %.3f' % (name, B.SEEDS[name], margin))
    assert margin >= 1


def test_one_shape_at_most_falls_back_to_relative_l2():
    assert len(B.RELATIVE_L2) <= 1 and set(B.SEEDS) == set(B.SHAPES) and set(B.GATE + B.ABI_ONLY) == set(B.SHAPES)

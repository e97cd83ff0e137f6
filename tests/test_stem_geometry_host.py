"""No GPU: the table of tests/stem_geometry_cases.py against the library's probes (node_stem_describe / node_trunk_describe), its
seed rule on the two CPU runs, and the boundary between the shapes the stem's kernels take and the ones they refuse."""
import ctypes as C

import pytest

from tests import stem_geometry_cases as G

NODE_ERR_NULL, NODE_ERR_SHAPE, NODE_ERR_UNSUPPORTED = -1, -2, -3


def test_probes_are_exported_and_bound():
    """(that the header declares exactly what the library exports is tests/test_host_and_abi.py's)"""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    for name in ('node_stem_describe', 'node_trunk_describe'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.node_abi_version() == 6 == _lib.NODE_ABI_VERSION          # additions only
    # six and 4 x 6 + 1 + 4 + 4 int32_t: node_stem_gn_info, node_stem_info
    assert C.sizeof(_lib.NodeStemGnInfo) == 24 and C.sizeof(_lib.NodeStemInfo) == 4 * 24 + 4 + 16 + 16
    info = _lib.NodeStemInfo()
    assert lib.node_stem_describe(C.byref(_lib.NodeStemShape(5, 3, 44, 44, 128, 1e-5)), C.byref(info)) == 0
    g = info.gn[1]
    assert (g.hw, g.channels, g.cpg, g.cb, g.blocks_per_sample, g.grid) == (441, 64, 2, 32, 2, 10)
    assert info.takes_w4 == 0 and list(info.wgrad_nsplit) == [28, 28, 8, 8] and list(info.wgrad_rows_per_split) == [80] * 4


def test_probes_report_the_refusal_codes_of_the_workspace_calls():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    St, Tr = _lib.NodeStemShape, _lib.NodeTrunkShape
    info, gn = _lib.NodeStemInfo(), _lib.NodeStemGnInfo()
    assert lib.node_stem_describe(None, C.byref(info)) == NODE_ERR_NULL
    assert lib.node_stem_describe(C.byref(St(2, 3, 32, 32, 64, 1e-5)), None) == NODE_ERR_NULL
    assert lib.node_trunk_describe(None, C.byref(gn)) == NODE_ERR_NULL
    assert lib.node_trunk_describe(C.byref(Tr(2, 64, 8, 8, 1, 1e-5)), None) == NODE_ERR_NULL
    for bad, code in ((St(0, 3, 32, 32, 64, 1e-5), NODE_ERR_SHAPE), (St(2, 3, 5, 4, 64, 1e-5), NODE_ERR_SHAPE),
                      (St(2, 4, 32, 32, 64, 1e-5), NODE_ERR_UNSUPPORTED), (St(2, 3, 32, 32, 24, 1e-5), NODE_ERR_UNSUPPORTED),
                      (St(2, 3, 32, 32, 192, 1e-5), NODE_ERR_UNSUPPORTED), (St(1, 3, 51, 51, 64, 1e-5), NODE_ERR_UNSUPPORTED)):
        info.takes_w4 = 7
        assert lib.node_stem_describe(C.byref(bad), C.byref(info)) == code and len(lib.node_last_error()) > 0
        assert info.takes_w4 == 0 and info.gn[0].cb == 0                  # zeroed
        assert lib.node_stem_workspace_bytes(C.byref(bad)) == 0
    for bad, code in ((Tr(0, 64, 8, 8, 1, 1e-5), NODE_ERR_SHAPE), (Tr(2, 96, 8, 8, 1, 1e-5), NODE_ERR_UNSUPPORTED),
                      (Tr(2, 64, 8, 8, 0, 1e-5), NODE_ERR_UNSUPPORTED), (Tr(1, 64, 49, 49, 1, 1e-5), NODE_ERR_UNSUPPORTED)):
        gn.cb = 7
        assert lib.node_trunk_describe(C.byref(bad), C.byref(gn)) == code and gn.cb == 0
        assert lib.node_trunk_workspace_bytes(C.byref(bad), 1) == 0


def test_the_probe_reports_the_shapes_the_older_tests_run():
    """tests/test_gpu_stem_gn_paths.py states these from a restatement of stem_gn_cb; here they come from the library."""
    from neural_ode_features_amd import _lib
    geom = lambda d: [(g['hw'], g['channels'], g['cpg'], g['cb'], g['grid']) for g in d['gn']]
    d = _lib.stem_plan(2, 3, 32, 32, 256)
    assert geom(d) == [(900, 64, 2, 16, 8), (225, 64, 2, 64, 2), (225, 64, 2, 64, 2), (64, 256, 8, 128, 4)] and not d['takes_w4']
    assert geom(_lib.stem_plan(2, 1, 28, 28, 64)) == [(676, 64, 2, 16, 8), (169, 64, 2, 64, 2), (169, 64, 2, 64, 2), (49, 64, 2, 64, 2)]
    assert geom(_lib.stem_plan(5, 3, 32, 32, 64))[0] == (900, 64, 2, 16, 20)
    assert _lib.stem_plan(8, 3, 32, 32, 256)['takes_w4'] and not _lib.stem_plan(8, 3, 32, 32, 64)['takes_w4']
    t = _lib.trunk_plan(2, 256, 8, 8, 2)
    assert (t['hw'], t['channels'], t['cpg'], t['cb'], t['blocks_per_sample'], t['grid']) == (64, 256, 8, 128, 2, 4)
    for d in (d, _lib.stem_plan(128, 3, 32, 32, 256)):
        for ns, rps in d['wgrad']:
            assert ns >= 1 and rps % 16 == 0


def test_takes_w4_follows_its_switch(monkeypatch):
    from neural_ode_features_amd import _lib
    monkeypatch.delenv('NODE_TUNE_STEM_W4', raising=False)
    assert _lib.stem_plan(8, 3, 31, 34, 128)['takes_w4']
    assert not _lib.stem_plan(8, 3, 31, 35, 128)['takes_w4']            # 29 x 33 -> 15 x 17 -> 8 x 9
    assert not _lib.stem_plan(2, 3, 32, 32, 1024)['takes_w4'] and not _lib.stem_plan(8, 3, 32, 32, 1024)['takes_w4']      # 16 % cpg
    monkeypatch.setenv('NODE_TUNE_STEM_W4', '0')
    assert not _lib.stem_plan(8, 3, 31, 34, 128)['takes_w4']


def test_the_table_reaches_what_it_claims():
    plans = G.check_coverage()
    assert set(plans) == set(G.CASES) and len(G.CASES) == len(G.STEM_ROWS) + 2 + len(G.TRUNK_ROWS)
    for case, p in plans.items():
        print(case, p)
    # the rows the issue names, by their regimes
    gn = lambda case: [g[:5] for g in plans[case]['gn']]
    assert gn('r51x47_f256') == [(2205, 64, 8, 8, 8), (575, 64, 32, 2, 2), (575, 64, 32, 2, 2), (156, 256, 64, 4, 4)]
    assert [g[4] for g in gn('s44_f128_n5')] == [40, 10, 10, 5]
    assert plans['s5_f256']['nsplit'] == [1, 1, 1, 1] and [g[0] for g in gn('s5_f256')] == [9, 4, 4, 1]
    assert plans['r31x34_f128_n8']['w4'] and not plans['r31x34_f128_n8/w4off']['w4']
    assert plans['s32_f512_n8/w4off']['gn'][3] == (64, 512, 128, 4, 32, 16)
    assert plans['s32_f1024_n2']['gn'][3] == (64, 1024, 128, 8, 16, 32) and not plans['s32_f1024_n2']['w4']


def test_the_ceiling_and_the_floor():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    St = _lib.NodeStemShape
    d = _lib.stem_plan(1, 3, 50, 52, 64)
    assert lib.node_stem_workspace_bytes(C.byref(St(1, 3, 50, 52, 64, 1e-5))) > 0
    hw, cb = d['gn'][0]['hw'], d['gn'][0]['cb']
    assert (hw, cb) == (2400, 8)
    assert (hw * cb + 512) * 4 <= 160 * 1024 and (2 * hw * cb + 1024) * 4 == 157696 <= 160 * 1024
    assert hw * cb * 2 * 4 == 150 * 1024                                  # stem_gn_cb's budget, met exactly
    for g in d['gn']:
        assert (2 * g['hw'] * g['cb'] + 1024) * 4 <= 160 * 1024
    for bad in (St(1, 3, 51, 51, 64, 1e-5), St(1, 3, 5, 4, 64, 1e-5), St(1, 3, 4, 5, 64, 1e-5), St(1, 3, 50, 52, 192, 1e-5),
                St(1, 3, 32, 32, 192, 1e-5), St(1, 3, 43, 61, 64, 1e-5)):          # (41 x 59 = 2419)
        assert lib.node_stem_workspace_bytes(C.byref(bad)) == 0, (bad.h, bad.w, bad.filters)
    assert lib.node_stem_workspace_bytes(C.byref(St(1, 3, 5, 5, 64, 1e-5))) > 0
    assert lib.node_stem_workspace_bytes(C.byref(St(1, 3, 42, 62, 64, 1e-5))) > 0          # 40 x 60 = 2400 the other way round
    # the trunk: the same budget on h w itself
    Tr = _lib.NodeTrunkShape
    assert lib.node_trunk_workspace_bytes(C.byref(Tr(1, 64, 48, 50, 1, 1e-5)), 1) > 0
    assert lib.node_trunk_workspace_bytes(C.byref(Tr(1, 64, 49, 49, 1, 1e-5)), 1) == 0


@pytest.mark.parametrize('name', list(G.STEM_ROWS) + list(G.TRUNK_ROWS))
def test_the_recorded_seed_meets_the_seed_rule(name):
    """No GroupNorm output of the float64 run within 8 x the float32 CPU run's distance of zero (both runs on the CPU; forward only).
    The seeds were searched for a margin of G.MARGIN[row] so that the rule holds with other fp32 kernels too; what is asserted on every
    host is the rule itself."""
    row = G.row_of(name)[1]
    assert isinstance(row['seed'], int) and row['seed'] >= 1
    assert G.MARGIN[name] >= (1 if name in G.LARGE else 2)
    margin = G.seed_margin(name)
    print('%s: seed %d, min |u| / (8 x fp32 distance) = %.3f (searched for %g)' % (name, row['seed'], margin, G.MARGIN[name]))
    assert margin >= 1

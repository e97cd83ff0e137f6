"""Which kernel instance a shape selects, asserted without a GPU: the whole table of tests/param_grad_cases.py (what
tests/test_gpu_param_grads.py and tests/test_gpu_forced_tiles.py claim to cover) against `node_describe_dims`, every switch set in
a child process of its own -- the library reads NODE_TUNE_WGRAD_* / NODE_TUNE_CONV_* once per process."""
import ctypes as C
import subprocess

import pytest

from tests import param_grad_cases as cases


@pytest.mark.parametrize('group', list(cases.GROUPS))
def test_every_row_selects_the_kernels_it_claims(group):
    r = subprocess.run(cases.child_command(group, select_only=True), env=cases.child_env(group), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'selection of group %s: %d rows as claimed' % (group, len(cases.GROUPS[group][1])) in r.stdout


def test_the_rows_cover_every_instance_of_both_selectors():
    """Every value of the NODE_WGRAD_* and NODE_CONV_* enums is reached by a row -- by default where a default shape exists, behind
    a switch otherwise -- or is listed in NOT_REACHED with its reason; and the names are the binding's, in the enums' order."""
    from neural_ode_features_amd import _lib
    assert tuple(_lib.WGRAD_KERNELS) == cases.WGRAD_KERNELS and tuple(_lib.CONV_KERNELS) == cases.CONV_KERNELS
    wg, cv = cases.check_coverage()
    for k in cases.WGRAD_KERNELS + cases.CONV_KERNELS:
        groups = (wg.get(k) or cv.get(k) or set())
        print('%-10s %s' % (k, ', '.join(sorted(groups)) if groups else 'NOT REACHED: ' + cases.NOT_REACHED[k]))
    # by default wherever the default selection can produce the instance at all: the Winograd-domain and templated wgrad instances
    # at 8x8 / 16x16 / 4x4 exist only behind NODE_TUNE_WGRAD_WINO (dims.hip prefers the 2-D Winograd domain wherever a unit size exists)
    assert {k for k, g in wg.items() if 'default' in g} == {'W2_8', 'W2_4', 'T_7_7', 'P'}
    assert {k for k, g in cv.items() if 'default' in g} == set(cases.CONV_KERNELS)


def test_describe_dims_reports_errors_and_fields():
    """node_describe_dims returns dims_for's error code for a shape the solver refuses (and NODE_ERR_NULL for a missing argument),
    fills plain int32 fields otherwise, and touches no device."""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    info = _lib.NodeDimsInfo()
    assert lib.node_describe_dims(None, C.byref(info)) == -1
    assert lib.node_describe_dims(C.byref(_lib.NodeShape(2, 64, 8, 8, 32, 1e-5)), None) == -1
    assert lib.node_describe_dims(C.byref(_lib.NodeShape(4, 30, 8, 8, 30, 1e-5)), C.byref(info)) == -3      # C % 4
    assert lib.node_describe_dims(C.byref(_lib.NodeShape(4, 64, 8, 8, 7, 1e-5)), C.byref(info)) == -2       # groups
    assert lib.node_describe_dims(C.byref(_lib.NodeShape(4, 64, 40, 40, 32, 1e-5)), C.byref(info)) == -3 and len(lib.node_last_error()) > 0
    with pytest.raises(_lib.NodeHipError):
        _lib.describe_dims(0, 64, 8, 8)
    d = _lib.describe_dims(128, 256, 8, 8)
    assert set(d) == {k for k, _ in _lib.NodeDimsInfo._fields_}
    assert d['bm'] in (64, 128, 256) and d['mtiles'] * d['s'] >= 128 and d['ntile'] == 4 and 1 <= d['nsplit'] <= 32
    assert d['wgrad_kernel'] in _lib.WGRAD_KERNELS and d['conv_kernel'] in _lib.CONV_KERNELS

"""One VJP of the dynamics (`odefunc_vjp`) against the fp64 oracle, block by block, on every fp32 weight-gradient and convolution
kernel instance.

The flat comparison of the parity tests is one max-norm over all 18 C^2 + 26 C parameter gradients divided by the largest of
them; here every block -- the six GroupNorm vectors, the two conv biases, the time-channel taps `w[:, 0]` and each of the nine
data taps `w[:, 1:, kh, kw]` of both conv weights, and vjp_t -- is held to the same number at its OWN scale (tests/helpers.py;
tests/test_param_blocks_host.py shows on the CPU which defects that separates).  The reference is the oracle's own code in float64
on the CPU.

Which kernel a case runs is asserted, not assumed: every case first checks through `node_describe_dims` the instances its row of
tests/param_grad_cases.py claims (tests/test_kernel_selection_host.py checks the whole table without a GPU, and that the rows
cover every value of both selectors).  Instances that only a once-per-process switch selects run in child processes, one at a
time; a child that crashes or hangs fails its test and no further child is started.

Parameters are ordinary (live ReLU masks) below 10^5 state elements and kink-free from there on, as in tests/test_gpu_parity.py.
NODE_PARAM_GRAD_TABLES=<file> appends every case's table to that file (profiles/param_grad_blocks.txt is such a run)."""
import subprocess

import pytest

from tests import param_grad_cases as cases

pytestmark = pytest.mark.gpu


def _id(r):
    return 'x'.join(map(str, r['shape']))


@pytest.mark.parametrize('r', cases.DEFAULT, ids=_id)
def test_default_selection_block_by_block(r):
    cases.assert_group_environment('default')
    misses = cases.run_case(r, 'default')
    assert not misses, (r['shape'], r['why'], misses)


@pytest.mark.parametrize('r', cases.W4, ids=_id)
def test_w4_pipeline_block_by_block(r):
    """The F(4x4,3x3) pipeline forced on (NODE_TUNE_WINO4=2, read per call), on bf16 triples and with the fp16 pairs allowed (a
    solve moves to the pairs after its first evaluations; a single evaluation may run the triples under both settings).  That the
    pipeline did run is checked against the same call with it off: another algorithm, other bits."""
    import torch
    cases.assert_group_environment('w4')
    misses, got = [], {}
    for f16 in ('0', '1'):
        got[f16] = {}
        misses += ['W4_F16=%s: %s' % (f16, m) for m in
                   cases.run_case(r, 'w4', env=dict(NODE_TUNE_WINO4='2', NODE_TUNE_W4_F16=f16), tag=' W4_F16=' + f16, keep=got[f16])]
    assert not misses, (r['shape'], r['why'], misses)
    off = {}
    assert not cases.run_case(dict(r, w4=0), 'w4', env=dict(NODE_TUNE_WINO4='0'), tag=' F(4x4,3x3) off', keep=off)
    assert not torch.equal(off['vp'], got['0']['vp']) and not torch.equal(off['vp'], got['1']['vp'])


_CRASHED = []          # the group whose child ended on a signal, an abort or its time limit: nothing more is started


@pytest.mark.parametrize('group', [g for g, _, _ in cases.CHILDREN])
def test_kernels_behind_the_switches_block_by_block(group):
    """The instances that only NODE_TUNE_WGRAD_WINO / _VARIANT / NODE_TUNE_CONV_WINO / _BM select (read once per process): the same
    check in a fresh child per switch set.  The child asserts its environment and every row's selection before its first launch."""
    assert not _CRASHED, 'not started: the child of group %r crashed or hung' % _CRASHED[0]
    try:
        r = subprocess.run(cases.child_command(group), env=cases.child_env(group), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _CRASHED.append(group)
        pytest.fail('child %s hit its time limit\n%s' % (group, (e.stdout or b'')[-2000:]))
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (134, 139):
        _CRASHED.append(group)
    assert r.returncode == 0, 'child %s: exit status %d\n%s\n%s' % (group, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count('  vjp_t ') == len(cases.GROUPS[group][1])          # every row ran

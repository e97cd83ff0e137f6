"""GPU parity of the fp16-PAIR kernels at long reductions (C = 512 and 1024: what configs[4] runs) INSIDE whole adjoint solves,
against the fp64 oracle.  Pairs run only in adaptive dopri5 solves whose virtual batch Nv (N; 4 N for 16 x 16 states) and width
pass w4_f16_fits (csrc/w4_select.hip): every single-evaluation test at C >= 512 runs the bf16-triple kernels instead, and the
convolution-only pair tests take their scales from k_w4_scales, not from the GroupNorm passes that set them in a solve.  Here a
free-running solve supplies the step sizes, and the same steps are replayed on the device and by the fp64 oracle
(tests.helpers.kink_free_replay): forward pair GEMMs, the cotangent-side exponent, k_w4_wgrad64h at (C / 128)^2 = 16 and 64 tiles
per component, the time-channel weight gradient and, on 16 x 16 states, the quadrant passes writing pair operands at 32 channels
per group.

Which kernel a case runs follows from launch_w4_gemm_f16: C >= 512 takes k_w4_gemm128h<2> (N % 32 == 0, even nT = (Nv / 32)(C / 128)),
and k_w4_gemm256h + the k_w4_gemm128h<2> tail for components 32..35 where Nv % 64 == 0 and nT2 = (Nv / 64)(C / 256) is a multiple
of 8 (NODE_TUNE_W4_H256 = 2: wherever Nv % 64 == 0); the weight gradient is k_w4_wgrad64h with T = (C / 128)^2 tiles per component.
C = 1024 runs the pipeline on 16 x 16 states only: 32 groups of 32 channels fit the quadrant passes, while the 8 x 8 passes hold
a group in one wave (16 % cpg == 0, csrc/dims.hip), so an 8 x 8 state at C = 1024 takes the fp32 F(2x2,3x3) kernels and no
pairs.  The tight 8 x 8 claims on k_w4_gemm256h are therefore made at C = 512.

16 x 16 states carry a known defect (profiles/r06_nondeterminism.txt: in < 1 % of solves a few (sample, channel % 16 == 5,
tile (1, 1)) units are off by up to 4e-3 of max|y|, or whole samples by up to 2e-4), so their claims are ones that a few bad units
cannot move but a wrong kernel would: the per-sample max-norm MEDIAN, relative L2 per tensor and an every-element ceiling of 1e-2.
Elements beyond the tight bound are counted and located in the log.  8 x 8 states have no quadrant passes and carry the tight
max-norm claims, the pairs-against-triples comparison and the free-running solve against its replay."""
import pytest
import torch

from tests.helpers import _arbiter_device, kink_free_replay, per_sample_err, rel_err

pytestmark = pytest.mark.gpu

# Bounds, each about 5 x the largest error measured over the cases on an MI355X (in parentheses) and under the issue-level ceilings
# (8 x 8 max norm: output 5e-5, gradients 2e-4; 16 x 16: relative L2 5e-4, every element 1e-2).
# 8 x 8, max norm relative to each tensor's largest entry:
OUT_TOL = 7e-6        # output (1.36e-6)
GRAD_TOL = 4e-5       # grad_y0 and each parameter tensor, time-channel slices included (7.8e-6, grad norm2.weight at C = 512)
CHAN_TOL = 1.2e-4     # conv weight gradients per output channel, relative to that channel's largest entry (2.5e-5)
REPLAY_TOL = 1e-6     # free-running solve against its own replay (bit-identical: 0)
# 16 x 16 (the known defect moves single units by up to 4e-3 of max|y|; a handful of them in the 2 M elements of an 8-sample state
# would move the relative L2 of the output by ~1e-4, hence the wider margin of the L2 bounds):
MEDIAN_TOL = 6e-6     # per-sample max-norm median of output and grad_y0 (1.12e-6)
L2_TOL = 2e-4         # relative L2 per tensor (1.9e-5, grad norm1.bias at (32, 1024, 16, 16))
CHAN_L2_TOL = 1e-3    # conv weight gradients, relative L2 per output channel (1.5e-4, conv1 at (32, 1024, 16, 16))
CEIL = 1e-2           # every element, relative to the tensor's largest entry: structural errors of O(1) (1.3e-5)


def _bound8(name):
    return OUT_TOL if name == 'out' else CHAN_TOL if name.endswith('per channel') else GRAD_TOL


CASES = [
    pytest.param((32, 512, 8, 8), {}, id='32x512x8x8-gemm128h2-wgrad64h_T16'),
    # H256 = 2 takes k_w4_gemm256h + tail at nT2 = 2; the case also replays under H256 = 0 (k_w4_gemm128h<2> at nT = 4)
    pytest.param((64, 512, 8, 8), {'NODE_TUNE_W4_H256': '2'}, id='64x512x8x8-H256_2-gemm256h_tail-wgrad64h_T16'),
    pytest.param((8, 1024, 16, 16), {}, id='8x1024x16x16-gemm128h2-quadrants_cpg32-wgrad64h_T64'),
    pytest.param((32, 1024, 16, 16), {}, id='32x1024x16x16-cfg5-gemm256h_tail-wgrad64h_T64'),
]


def _tensors(r):
    """(name, hip-side tensor) pairs to check: output, grad_y0, the ten parameter gradients, and the time channel w[:, 0] of both
    convolutions on its own scale (it comes from the time-channel weight-gradient kernel, not from k_w4_wgrad64h)."""
    out = [('out', r['out']), ('grad_y0', r['gy'])]
    out += [('grad ' + n, g) for n, g in r['gp'].items()]
    out += [('grad ' + n + '[:, 0]', g[:, 0]) for n, g in r['gp'].items() if g.dim() == 4]
    return out


def _errors(r, ref):
    """max-norm error relative to the reference tensor's largest entry, per tensor; conv weights also per output channel."""
    e = {}
    for (name, a), (_, b) in zip(_tensors(r), _tensors(ref)):
        e[name] = rel_err(a, b)
        if name.startswith('grad conv') and name.endswith('weight'):
            d = (a.double() - b.double()).abs().flatten(1).amax(dim=1) / b.double().abs().flatten(1).amax(dim=1)
            e[name + ' per channel'] = float(d.max())
    return e


def _l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _locate(name, a, b, bound):
    """16 x 16 states: how many elements exceed the tight bound, and where (channel % 16, 4 x 4 tile in the 8 x 8 quadrant) --
    the signature of the known nondeterminism, printed so that its fix can tighten these tests."""
    a, b = a.double(), b.double()
    bad = (a - b).abs() > bound * b.abs().max()
    n = int(bad.sum())
    if n and a.dim() == 4:
        _, c, h, w = bad.nonzero(as_tuple=True)
        where = {}
        for k in zip((c % 16).tolist(), ((h % 8) // 4).tolist(), ((w % 8) // 4).tolist()):
            where[k] = where.get(k, 0) + 1
        print('   %s: %d elements beyond %.0e of max; (channel %% 16, tile in quadrant): count %s' % (name, n, bound, sorted(where.items())))
    elif n:
        print('   %s: %d elements beyond %.0e of max' % (name, n, bound))


def _check_solve(r, tag, replay=True):
    """The NFE law: 2 + 6 steps forward, 3 + 6 steps backward (model.py:340 counting); a replay skips the initial step-size
    selection and its one evaluation in each direction."""
    fs, bs = r['fwd'], r['bwd']
    print('  %s: pair stats %s, forward %s, backward %s' % (tag, r['pair'], (fs['accepted'], fs['rejected'], fs['nfe']),
                                                         (bs['accepted'], bs['rejected'], bs['nfe'])))
    assert fs['nfe'] == 2 - replay + 6 * (fs['accepted'] + fs['rejected']), fs
    assert bs['nfe'] == 3 - replay + 6 * (bs['accepted'] + bs['rejected']), bs
    assert r['nfe'] == fs['nfe'] + bs['nfe']
    if replay:
        assert fs['rejected'] == 0 and bs['rejected'] == 0


@pytest.mark.parametrize('shape,env', CASES)
def test_wide_pair_solve_replay_against_fp64(shape, env):
    """A kink-free adjoint solve (tol 1e-3, t in [0, 1]) on the fp16-pair kernels at C = 512 / 1024, replayed by the fp64 oracle on
    the same steps.  Every case: pairs ran and no step was repeated; the NFE law in both directions; output, grad_y0, every
    parameter gradient, every conv weight gradient per output channel and the time-channel slices against fp64.
    8 x 8: max norm (bounds and measured errors above); the same replay on bf16 triples (NODE_TUNE_W4_F16 = 0) bounds the pairs'
    error per tensor at 2 x the triples' + 1e-6 (measured: the pairs' at or below the triples' but for grad norm2.weight, 7.8e-6
    against 7.4e-6); the free-running solve reproduces its replay bit for bit.  (64, 512, 8, 8)
    with H256 = 2 also replays under H256 = 0: components 32..35 are reduced differently there, so the two must NOT be bit-identical
    (the switch took effect; measured: outputs 1.8e-6 apart), and both meet the bounds.  16 x 16: per-sample max-norm median of
    output and grad_y0, relative L2 per tensor and per conv output channel, every element under the ceiling; elements beyond the
    8 x 8 bound are located in the log (measured: none).  Each case takes 1 - 4 s with the fp64 replay on the device."""
    N, C, H, W = shape
    if C >= 1024 and _arbiter_device() != 'cuda':
        pytest.skip('no fp64 convolution on the device: the fp64 replay at C = 1024 on the host takes minutes')
    wide8 = H == 8
    envs = [dict(env)]
    if wide8:
        envs.append(dict(env, NODE_TUNE_W4_F16='0'))
    if env.get('NODE_TUNE_W4_H256') == '2':
        envs.append(dict(env, NODE_TUNE_W4_H256='0'))
    free, reps, f64 = kink_free_replay(shape, envs, tol=1e-3, seed=53, t_end=1.0)
    _check_solve(free, 'free-running', replay=False)
    assert free['pair'][0] == 1 and free['pair'][1] == 0, free['pair']
    hip = reps[0]
    _check_solve(hip, 'pairs')
    assert (hip['fwd']['accepted'], hip['bwd']['accepted']) == (free['fwd']['accepted'], free['bwd']['accepted'])
    assert hip['pair'][0] == 1 and hip['pair'][1] == 0, hip['pair']      # pairs were used; no step had to be repeated
    e = _errors(hip, f64)
    if wide8:
        tri = reps[1]
        _check_solve(tri, 'triples')
        assert tri['pair'][0] == 0, tri['pair']
        e3 = _errors(tri, f64)
        for k in e:
            print('  %-32s pairs %.2e  triples %.2e' % (k, e[k], e3[k]))
        for k in e:
            assert e[k] <= _bound8(k), (k, e[k])
            assert e[k] <= 2 * e3[k] + 1e-6, (k, e[k], e3[k])
        ef = _errors(free, hip)
        print('  free-running vs its replay: max %.2e' % max(ef.values()))
        assert all(v <= REPLAY_TOL for v in ef.values()), ef
        if len(reps) > 2:
            other = reps[2]
            _check_solve(other, 'H256=0')
            assert other['pair'][0] == 1 and other['pair'][1] == 0, other['pair']
            eo = _errors(other, f64)
            print('  H256=0 replay: max error %.2e (output %.2e); |H256=2 - H256=0| output %.2e'
                  % (max(eo.values()), eo['out'], rel_err(hip['out'], other['out'])))
            assert not torch.equal(hip['out'], other['out'])      # components 32..35 reduced another way: the switch took effect
            for k in eo:
                assert eo[k] <= _bound8(k), (k, eo[k])
    else:
        for (name, a), (_, b) in zip(_tensors(hip), _tensors(f64)):
            l2 = _l2(a, b)
            line = '  %-32s max %.2e  L2 %.2e' % (name, e[name], l2)
            if name in ('out', 'grad_y0'):
                med = float(per_sample_err(a, b).median())
                line += '  per-sample median %.2e' % med
                assert med <= MEDIAN_TOL, (name, med)
            if name + ' per channel' in e:
                pc = float(((a.double() - b.double()).flatten(1).norm(dim=1) / b.double().flatten(1).norm(dim=1)).max())
                line += '  per-channel L2 max %.2e' % pc
                assert pc <= CHAN_L2_TOL, (name, pc)
            print(line)
            _locate(name, a, b, _bound8(name))
            assert l2 <= L2_TOL, (name, l2)
            assert e[name] <= CEIL, (name, e[name])

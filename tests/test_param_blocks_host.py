"""The block-wise comparison of parameter gradients (tests/helpers.py: param_grad_blocks, block_errors, odefunc_vjp_ref64), checked
on the CPU: (1) the fp32 CPU oracle sits far inside the GPU tests' per-block bound at every shape they use, so that bound measures
the kernels and not the reference; (2) defects that the flat `rel_err(vp, vp_ref) < 5e-5` assertion provably passes are each
reported, in the right block."""
import pytest
import torch

from oracle.dynamics import odefunc_vjp as oracle_vjp
from tests import param_grad_cases as cases
from tests.helpers import block_errors, make_func, odefunc_vjp_ref64, param_grad_blocks, rel_err, vjp_block_errors

ROWS = {}
for _g, (_e, _rows) in cases.GROUPS.items():
    for _r in _rows:
        ROWS.setdefault((_r['shape'], cases.kink_free(_r)), _r)


def _oracle_pair(r, t=-0.61):
    N, C, H, W = r['shape']
    y, cot, ref = cases.reference(r, t)
    _, twin = make_func(C, seed=C + H, kink_free=cases.kink_free(r))
    _, _, vt32, vp32 = oracle_vjp(t, y, dict(twin.named_parameters()), cot)
    return ref, vp32, vt32


@pytest.mark.parametrize('key', list(ROWS), ids=lambda k: 'x'.join(map(str, k[0])) + ('-kinkfree' if k[1] else ''))
def test_fp32_oracle_is_far_inside_the_block_bound(key):
    """Every block of the fp32 CPU oracle's gradient (and vjp_t) within 5e-6 of the fp64 one, relative to the block's scale:
    a tenth of the 5e-5 the GPU tests allow.  (Measured: at most 2.8e-6, at [2, 64, 32, 32]; 2.3e-6 at the kink-free 8x8 shapes, under 1e-6 with ordinary parameters.)"""
    ref, vp32, vt32 = _oracle_pair(ROWS[key])
    errs = vjp_block_errors(vp32, vt32, ref)
    worst = max(errs, key=errs.get)
    print(key, 'worst block', worst, '%.2e' % errs[worst])
    assert errs[worst] < 5e-6, (worst, errs[worst])


def test_blocks_partition_the_flat_vector():
    """Every one of the 18 C^2 + 26 C gradients lies in exactly one block, in the PyTorch layout [co][1 + ci][kh][kw]."""
    C = 8
    flat = torch.arange(18 * C * C + 26 * C, dtype=torch.float64)
    b = param_grad_blocks(flat, C)
    assert len(b) == 6 + 2 + 2 * 10
    allv = torch.cat([v.reshape(-1) for v in b.values()])
    assert torch.equal(allv.sort().values, flat)
    w1 = flat[2 * C:2 * C + 9 * C * (C + 1)].reshape(C, C + 1, 3, 3)
    assert torch.equal(b['conv1.w_t'], w1[:, 0]) and torch.equal(b['conv1.tap21'], w1[:, 1:, 2, 1]) and b['conv2.bias'].shape == (C,)
    as_dict = {'norm1.weight': flat[:C], 'norm1.bias': flat[C:2 * C], 'conv1._layer.weight': w1}
    o = 2 * C + w1.numel()
    for k, n in (('conv1._layer.bias', C), ('norm2.weight', C), ('norm2.bias', C), ('conv2._layer.weight', w1.numel()),
                 ('conv2._layer.bias', C), ('norm3.weight', C), ('norm3.bias', C)):
        as_dict[k] = flat[o:o + n].reshape(w1.shape if n == w1.numel() else (C,))
        o += n
    b2 = param_grad_blocks(as_dict, C)
    assert all(torch.equal(b[k], b2[k]) for k in b)


# ---- planted defects ---------------------------------------------------------------------------------------------------------
KF = dict(shape=(130, 64, 8, 8))           # kink-free by size: the shape at which the blocks' scales differ most
FLAT_BOUND = BLOCK_BOUND = 5e-5


@pytest.fixture(scope='module')
def kf():
    ref, vp32, vt32 = _oracle_pair(KF)
    return ref, vp32.double(), float(vt32)


def _verdict(ref, vp, vt):
    """(flat rel_err against the fp64 gradient, the blocks over the bound)."""
    errs = vjp_block_errors(vp, vt, ref)
    return rel_err(vp, ref['vp']), {k: e for k, e in errs.items() if e > BLOCK_BOUND}


def _weight_view(vp, C, layer):
    o = 2 * C if layer == 1 else 2 * C + 9 * C * (C + 1) + 3 * C
    return vp[o:o + 9 * C * (C + 1)].view(C, C + 1, 3, 3)


def test_clean_gradient_reports_nothing(kf):
    ref, vp, vt = kf
    flat, over = _verdict(ref, vp, vt)
    assert flat < FLAT_BOUND and over == {}


def test_scaled_time_channel_tap_is_reported(kf):
    """One tap of conv1's time-channel sums off by 0.3 % (a wrong border mask in that tap's sum): 3e-3 of a block that is ~1e-2 of
    the largest gradient."""
    ref, vp, vt = kf
    bad = vp.clone()
    _weight_view(bad, 64, 1)[:, 0, 1, 1] *= 1 + 3e-3
    flat, over = _verdict(ref, bad, vt)
    print('flat', flat, over)
    assert flat < FLAT_BOUND, flat
    assert set(over) == {'conv1.w_t'} and over['conv1.w_t'] > 10 * BLOCK_BOUND


def test_lost_corner_tap_element_is_reported(kf):
    """A corner data tap zeroed for a single (co, ci) -- a lost split-K slab of one output element -- whose magnitude is under 5e-5
    of the largest gradient: invisible to the flat comparison whatever the value, visible at the tap's own scale."""
    ref, vp, vt = kf
    gmax = float(ref['vp'].abs().max())
    w = ref['blocks']['conv1.tap00']
    scale = float(w.abs().max())
    cand = w.abs().clone()
    cand[cand >= 0.9 * FLAT_BOUND * gmax] = 0
    co, ci = divmod(int(cand.argmax()), w.shape[1])
    assert 2 * BLOCK_BOUND * scale < float(cand[co, ci]) < FLAT_BOUND * gmax, (float(cand[co, ci]), scale, gmax)
    bad = vp.clone()
    _weight_view(bad, 64, 1)[co, 1 + ci, 0, 0] = 0
    flat, over = _verdict(ref, bad, vt)
    print('flat', flat, over, 'element', (co, ci), float(cand[co, ci]) / gmax)
    assert flat < FLAT_BOUND, flat
    assert set(over) == {'conv1.tap00'}


def test_norm1_bias_off_by_a_third_of_a_percent_is_reported(kf):
    ref, vp, vt = kf
    bad = vp.clone()
    bad[64:128] *= 1 + 3e-3
    flat, over = _verdict(ref, bad, vt)
    print('flat', flat, over)
    assert flat < FLAT_BOUND, flat
    assert set(over) == {'norm1.bias'} and over['norm1.bias'] > 10 * BLOCK_BOUND


def test_swapped_time_channel_taps_are_reported(kf):
    """Two taps of `w[:, 0]` swapped (a [tap][co] -> [co][0][kh][kw] permutation slip) where it shows least: the output channel
    and pair of taps of conv1 whose values differ least while still differing by more than twice the block bound."""
    ref, vp, vt = kf
    gmax = float(ref['vp'].abs().max())
    wt = ref['blocks']['conv1.w_t'].reshape(64, 9)
    scale = float(wt.abs().max())
    diff = (wt[:, :, None] - wt[:, None, :]).abs()
    diff[diff < 4 * BLOCK_BOUND * scale] = float('inf')
    co, rest = divmod(int(diff.argmin()), 81)
    a, b = divmod(rest, 9)
    assert 4 * BLOCK_BOUND * scale <= float(diff[co, a, b]) < 0.5 * FLAT_BOUND * gmax, (float(diff[co, a, b]), scale, gmax)
    bad = vp.clone()
    v = _weight_view(bad, 64, 1)[co, 0].view(9)
    v[a], v[b] = float(v[b]), float(v[a])
    flat, over = _verdict(ref, bad, vt)
    print('flat', flat, over, (co, a, b))
    assert flat < FLAT_BOUND, flat
    assert set(over) == {'conv1.w_t'}


def test_cancelled_sums_are_scaled_by_their_terms():
    """One channel per group (C <= 32): the GroupNorm behind each conv removes its bias exactly, so the true bias gradient is zero
    and max |ref| is no scale; the helper's scale is the sum of the cotangent magnitudes.  vjp_t likewise is scaled by the sum of
    its terms' magnitudes, which its own magnitude can fall far below."""
    r = dict(shape=(2, 32, 16, 16))
    ref, vp32, vt32 = _oracle_pair(r)
    for k in ('conv1.bias', 'conv2.bias'):
        assert float(ref['blocks'][k].abs().max()) < 1e-9 * ref['scales'][k], (k, float(ref['blocks'][k].abs().max()), ref['scales'][k])
    assert ref['scales']['vjp_t'] >= abs(ref['vt'])
    errs = vjp_block_errors(vp32, vt32, ref)
    assert errs['conv1.bias'] < 5e-6 and errs['conv2.bias'] < 5e-6 and errs['vjp_t'] < 5e-6
    # the identity behind vjp_t's scale
    p64 = ref['blocks']
    _, twin = make_func(32, seed=32 + 16)
    w = dict(twin.named_parameters())
    t32 = float(torch.tensor(-0.61, dtype=torch.float32))
    s = sum(float((w['conv%d._layer.weight' % l][:, 0].detach().double() * p64['conv%d.w_t' % l]).sum()) for l in (1, 2)) / t32
    assert abs(s - ref['vt']) <= 1e-12 * ref['scales']['vjp_t']

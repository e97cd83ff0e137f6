"""GPU: the set-up and tear-down of a solve as jobs of launches that exist anyway -- the border maps in the F(4x4,3x3) blocking and the
scalar setters in the preparation launch, y0's copies in the state's layout launch, the adjoint's two state conversions as one
launch, a deferred solve's record in its last step's commit.  What the separate launches left behind is what these must leave:
every comparison is torch.equal."""
import ctypes as C

import pytest
import torch

from tests.deferred_record import new_record, read_record
from tests.helpers import make_func

pytestmark = pytest.mark.gpu

_FUNCS = {}
# the issue's two layout shapes, and a 16x16 shape that an F(4x4,3x3) SOLVE takes (C % 128 == 0); the layout and map launches
# themselves take any C % 16 == 0, so all three run the kernels under test through the diagnostics entries
LAYOUT_SHAPES = [(3, 64, 8, 8), (2, 64, 16, 16), (2, 128, 16, 16)]


def _func(C_):
    if C_ not in _FUNCS:
        _FUNCS[C_] = make_func(C_, seed=41, device='cuda')[0]
    return _FUNCS[C_]


def _ids(s):
    return 'x'.join(map(str, s))


def _shape_struct(shape):
    from neural_ode_features_amd import _lib
    N, Cc, H, W = shape
    return _lib.NodeShape(N, Cc, H, W, min(32, Cc), 1e-5)


def _layout(shape, src, to_nchw=0):
    from neural_ode_features_amd import _lib
    dst = torch.full_like(src, float('nan'))
    _lib.check(_lib.load().node_w4s_layout(C.byref(_shape_struct(shape)), src.data_ptr(), dst.data_ptr(), to_nchw,
                                           torch.cuda.current_stream().cuda_stream))
    return dst


def _layout_jobs(shape, srcs, ncopies):
    """(dst per job, copies per job) of ONE k_w4s_layout_jobs launch; job i gets ncopies[i] straight-copy destinations."""
    from neural_ode_features_amd import _lib
    n = len(srcs)
    dsts = [torch.full_like(s, float('nan')) for s in srcs]
    copies = [[torch.full_like(s, float('nan')) for _ in range(k)] for s, k in zip(srcs, ncopies)]
    vp = C.c_void_p
    a_src = (vp * 2)(*[s.data_ptr() for s in srcs])
    a_dst = (vp * 2)(*[d.data_ptr() for d in dsts])
    flat = []
    for i in range(2):
        for k in range(2):
            flat.append(copies[i][k].data_ptr() if i < n and k < len(copies[i]) else None)
    a_cp = (vp * 4)(*flat)
    _lib.check(_lib.load().node_w4s_layout_jobs(C.byref(_shape_struct(shape)), n, a_src, a_dst, a_cp, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return dsts, copies


@pytest.mark.parametrize('shape', LAYOUT_SHAPES, ids=_ids)
def test_state_layout_launches_round_trip(shape):
    """k_w4s_layout_jobs against the one-tensor launch it replaces, element for element: one job with two, one and no copies (the
    forward solve's launch), two jobs (the adjoint's), two jobs with copies on the second; every state tensor equals what
    launch_w4s_from_nchw writes, every copy equals its job's source, and the old launch converts every state tensor back to its
    source.  Buffers start as NaN: an element nobody wrote cannot pass."""
    gen = torch.Generator().manual_seed(9)
    a = torch.randn(*shape, generator=gen).cuda()
    b = torch.randn(*shape, generator=gen).cuda()
    ref_a, ref_b = _layout(shape, a), _layout(shape, b)
    assert torch.equal(_layout(shape, ref_a, to_nchw=1), a) and not torch.equal(ref_a, a)
    for srcs, ncopies in (([a], [2]), ([a], [1]), ([a], [0]), ([a, b], [0, 0]), ([a, b], [1, 2]), ([b, a], [2, 0])):
        dsts, copies = _layout_jobs(shape, srcs, ncopies)
        for s, d, cps in zip(srcs, dsts, copies):
            assert torch.equal(d, ref_a if s is a else ref_b), (ncopies, 'state')
            assert torch.equal(_layout(shape, d, to_nchw=1), s), (ncopies, 'round trip')
            for cp in cps:
                assert torch.equal(cp, s), (ncopies, 'copy')


def _tmap_blocking(tmap, shape):
    """tmap [HW][C] -> the blocking the forward passes read: [Q quadrants][C/16][4 i][64 lanes = 16 t + c15][4 j], element =
    pixel (8 QY + 4 ty + i, 8 QX + 4 tx + j) of channel 16 cb + c15 (q = 2 QY + QX, t = 2 ty + tx; kernels_w4s.hip)."""
    _, Cc, H, W = shape
    Q, CB = (4 if H == 16 else 1), Cc // 16
    idx = torch.arange(64 * Q * Cc, device=tmap.device)
    j, lane, i, rest = idx & 3, (idx >> 2) & 63, (idx >> 8) & 3, idx >> 10
    q, cb = rest // CB, rest % CB
    t, c = lane >> 4, cb * 16 + (lane & 15)
    p = (8 * (q >> 1) + 4 * (t >> 1) + i) * W + 8 * (q & 1) + 4 * (t & 1) + j
    return tmap.reshape(-1)[p * Cc + c]


@pytest.mark.parametrize('shape', LAYOUT_SHAPES, ids=_ids)
def test_border_maps_in_the_pass_blocking(shape):
    """The preparation launch writes both layers' border maps twice: [HW][C] (jobs 0, 1) and in the passes' blocking (the jobs that
    replaced the permuting launch).  The blocked map must be the plain one permuted, bit for bit, for both layers -- and the plain
    one is the masked nine-tap sum of the time channel's filter taps (fp64 reference, fp32 rounding of nine terms)."""
    from neural_ode_features_amd import _lib
    N, Cc, H, W = shape
    f = _func(Cc)
    w1 = f.conv1._layer.weight.detach().contiguous()
    w2 = f.conv2._layer.weight.detach().contiguous()
    tmap = torch.full((2, H * W, Cc), float('nan'), device='cuda')
    tmap_s = torch.full((2, H * W * Cc), float('nan'), device='cuda')
    _lib.check(_lib.load().node_w4s_tmaps(C.byref(_shape_struct(shape)), w1.data_ptr(), w2.data_ptr(), tmap.data_ptr(), tmap_s.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for layer, w in enumerate((w1, w2)):
        assert torch.equal(tmap_s[layer], _tmap_blocking(tmap[layer], shape)), layer
        ones = torch.ones(1, 1, H, W, dtype=torch.float64)
        ref = torch.nn.functional.conv2d(ones, w[:, :1].double().cpu(), padding=1)[0].reshape(Cc, H * W).t()      # [HW][C], on the CPU
        scale = float(w[:, 0].abs().sum(dim=(1, 2)).max())
        assert float((tmap[layer].double().cpu() - ref).abs().max()) <= 9 * 2.0 ** -24 * scale
    assert not torch.equal(tmap_s[0], tmap_s[1])


def _forward(shape, tol=1e-3, steps=None, scale=1.0, seed=5):
    from neural_ode_features_amd import _lib, integrate
    f = _func(shape[1])
    rec = integrate.Recognised(f)
    y = scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()
    blind = recs = flag = None
    if steps is not None:
        recs = new_record()
        flag = torch.zeros(1, dtype=torch.float32, device='cuda')
        blind = (steps, recs, flag)
    out, st = integrate.solve_forward(rec, rec.params, y, [0.0, 1.0], tol, tol, _lib.METHODS['dopri5'], None, blind=blind)
    torch.cuda.synchronize()
    return y, out, st, (read_record(recs) if recs is not None else None), (float(flag) if flag is not None else None)


# F(4x4,3x3) solves (Q = 1, Q = 4) -- the layout launch with copies -- and one NHWC solve, whose copy stays a copy
@pytest.mark.parametrize('shape', [(3, 64, 8, 8), (16, 128, 8, 8), (2, 128, 16, 16), (2, 64, 16, 16)], ids=_ids)
def test_forward_solve_leaves_y0_in_the_first_slot(shape):
    y, out, st, _, _ = _forward(shape)
    assert torch.equal(out[0], y)
    assert bool(torch.isfinite(out[1]).all()) and not torch.equal(out[1], y)


@pytest.mark.parametrize('shape', [(16, 128, 8, 8), (2, 128, 16, 16)], ids=_ids)
def test_deferred_hit_and_miss_records(shape):
    """A hit: the record of a deferred solve with the exact step count equals what the synchronous solve reports.  A miss (one step
    too few): miss = 1, the flag goes up by one, done = 0, and the output slot holds y0, not whatever the allocation held."""
    y, out, st, _, _ = _forward(shape, tol=1e-5, scale=4.0)
    n = st['accepted'] + st['rejected']
    assert n >= 2
    y2, out_hit, _, rec, flag = _forward(shape, tol=1e-5, scale=4.0, steps=n)
    assert flag == 0.0 and rec['miss'] == 0 and rec['done'] == 1 and rec['status'] == 0
    assert (rec['steps'], rec['accepted'], rec['rejected']) == (n, st['accepted'], st['rejected'])
    assert rec['t'] == st['t_final'] >= 1.0 and rec['first_dt'] == st['first_dt']      # (t: the end of the last step, at or past the target)
    assert torch.equal(out_hit, out)
    y3, out_miss, _, rec, flag = _forward(shape, tol=1e-5, scale=4.0, steps=n - 1)
    assert flag == 1.0 and rec['miss'] == 1 and rec['done'] == 0 and rec['steps'] == n - 1
    assert torch.equal(out_miss[0], y3) and torch.equal(out_miss[1], y3)

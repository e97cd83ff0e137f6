"""GPU: the operand ring of the stem's two matrix kernels (csrc/kernels_stem.hip: k_stem_conv, k_stem_wgrad) at the shapes
where a ring can go wrong -- K loops shorter than, equal to and longer than its depth and no multiple of it, a ragged last
K step, several splits with a shorter last one, every pixel class of the stride-2 data gradient.

The ring changes WHEN an operand arrives, never the order in which products enter an accumulator, so every result must be
the same bits as the one-step schedule's (NODE_TUNE_STEM_RING=0): a read that beats its DMA shows up as a mismatch against
NaN-filled buffers, not as noise.  Accuracy is held against fp64 `F.conv2d` at the bound of
test_gpu_stem.py::test_stem_convolutions_match_fp64."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# ((cin, cout, image side, kernel, stride, pad), batch) -- K chunks of the convolution are (tap, 32 channels) in the ring and
# (tap, 64 channels) in the one-step schedule; K steps of the weight gradient are 16 pixels of the output
CASES = [
    ((64, 64, 5, 1, 2, 0), 2),       # 1x1: one tap x 64 channels (2 ring chunks: shorter than the ring); 18 rows
    ((128, 64, 5, 1, 1, 0), 1),      # 1x1 on 128 channels (4 chunks: the ring's depth + 1)
    ((64, 64, 5, 3, 2, 1), 1),       # 3x3 stride 2 at side 5: data-gradient classes of 1, 2, 2, 4 taps; weight gradient 9 rows = 1 ragged K step
    ((64, 64, 5, 3, 2, 1), 2),       # 18 rows: 2 K steps, the last ragged
    ((64, 64, 5, 3, 2, 1), 4),       # 36 rows: 3 K steps (the ring's depth)
    ((64, 64, 5, 3, 2, 1), 8),       # 72 rows: 5 K steps, the last ragged
    ((64, 64, 15, 3, 2, 1), 1),      # the four classes at side 15: more than one row tile
    ((64, 64, 15, 3, 1, 1), 1),      # 225 rows: three splits of 80 / 80 / 65
    ((256, 64, 5, 3, 1, 1), 2),      # 3x3 on 256 channels: 72 ring chunks
]


@functools.lru_cache(maxsize=None)
def _problem(geom, n):
    cin, cout, side, k, stride, pad = geom
    gen = torch.Generator().manual_seed(1000 * cin + 10 * side + k + n)
    x = torch.randn(n, cin, side, side, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) / (cin * k * k) ** 0.5
    yside = (side + 2 * pad - k) // stride + 1
    dy = torch.randn(n, cout, yside, yside, generator=gen)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    y_ref = F.conv2d(xd, wd, None, stride, pad)
    dx_ref, dw_ref = torch.autograd.grad(y_ref, (xd, wd), dy.double())
    return x.cuda(), w.cuda(), dy.cuda(), (y_ref.detach(), dx_ref, dw_ref)


def _one_conv(what, geom, n, x, w, dy):
    """node_stem_conv as tests/test_gpu_stem.py::_one_conv calls it, on a result AND a workspace freshly filled with NaNs"""
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    cin, cout, side, k, stride, pad = geom
    g = _lib.NodeConvGeom(n, cin, cout, side, side, k, stride, pad)
    nbytes = lib.node_stem_conv_workspace_bytes(C.byref(g))
    assert nbytes > 0, lib.node_last_error()
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device='cuda')     # 0xFFFF bf16 and 0xFFFFFFFF fp32 are NaNs
    yside = (side + 2 * pad - k) // stride + 1
    shape = {0: (n, cout, yside, yside), 1: (n, cin, side, side), 2: (cout, cin, k, k)}[what]
    res = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.node_stem_conv(C.byref(g), what, ptr(x), ptr(w), ptr(dy), res.data_ptr(), (ws.data_ptr() + 255) & ~255, nbytes,
                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return res.cpu()


@pytest.mark.parametrize('what', [0, 1, 2], ids=['forward', 'data_gradient', 'weight_gradient'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'c%d-%d_s%d_k%d_st%d_n%d' % (c[0][:5] + (c[1],)))
def test_ring_equals_the_one_step_schedule_and_matches_fp64(case, what, monkeypatch):
    geom, n = case
    x, w, dy, refs = _problem(geom, n)
    args = ((x, w, None), (None, w, dy), (x, None, dy))[what]
    for rep in range(3):
        monkeypatch.setenv('NODE_TUNE_STEM_RING', '0')
        one_step = _one_conv(what, geom, n, *args)
        monkeypatch.delenv('NODE_TUNE_STEM_RING')
        ring = _one_conv(what, geom, n, *args)
        assert not torch.isnan(ring).any() and not torch.isnan(one_step).any(), (geom, n, what, rep)
        assert torch.equal(ring, one_step), (geom, n, what, rep, float((ring - one_step).abs().max()))
    ref = refs[what]
    err = float((ring.double() - ref).abs().max() / ref.abs().max())
    print('geom %s n %d what %d: max error / max|ref| = %.2e' % (geom, n, what, err))
    assert err <= 1e-5, (geom, n, what, err)

"""GPU: the 4x4 / stride 2 / padding 1 geometry of the stem's kernel family (csrc/kernels_stem.hip) -- the down-sampling
convolution of the `convolution` and `ode2` stems (model.py:148-164, 199-223) -- alone, through `node_stem_conv`:
forward (one class of 16 taps), data gradient (four parity classes of four taps) and weight gradient (k_stem_wgrad<4>: one
kernel row of four taps per workgroup) against an fp64 `F.conv2d`.

The bound is the family's own 1e-5 of max|ref| (tests/test_gpu_stem.py::test_stem_convolutions_match_fp64): the arithmetic is
the same -- exact bf16 triples, fp32 accumulation -- with the reduction growing from K = 2304 to K = 4096 at 256 channels.
Result and workspace start out as NaNs (tests/test_gpu_stem_pipeline.py), and the operand ring must give the bits of the
one-step schedule (NODE_TUNE_STEM_RING=0)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (cin, cout, image side, kernel, stride, pad)
GEOMS = [(64, 64, 30, 4, 2, 1),      # even side: the last tap row / column falls into the padding
         (64, 256, 15, 4, 2, 1),     # odd side -> 7
         (256, 256, 16, 4, 2, 1),    # the CIFAR hand-off of the `ode2` stem
         (64, 64, 6, 4, 2, 1)]       # 9 output pixels per image: fewer rows than one split share of the weight gradient


@functools.lru_cache(maxsize=None)
def _problem(geom, n):
    cin, cout, side, k, stride, pad = geom
    gen = torch.Generator().manual_seed(1000 * cin + 10 * side + cout + n)
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
@pytest.mark.parametrize('n', [3, 8])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'c%d-%d_s%d' % g[:3])
def test_conv4_matches_fp64_and_the_one_step_schedule(geom, n, what, monkeypatch):
    """n = 3: row counts that are no multiple of the 128-row tile or of the weight gradient's 16-pixel K step."""
    x, w, dy, refs = _problem(geom, n)
    args = ((x, w, None), (None, w, dy), (x, None, dy))[what]
    monkeypatch.setenv('NODE_TUNE_STEM_RING', '0')
    one_step = _one_conv(what, geom, n, *args)
    monkeypatch.delenv('NODE_TUNE_STEM_RING')
    ring = _one_conv(what, geom, n, *args)
    assert not torch.isnan(ring).any() and not torch.isnan(one_step).any(), (geom, n, what)
    ref = refs[what]
    err = float((ring.double() - ref).abs().max() / ref.abs().max())
    print('conv4 geom %s n %d what %d: max error / max|ref| = %.2e' % (geom, n, what, err))
    assert err <= 1e-5, (geom, n, what, err)
    assert torch.equal(ring, one_step), (geom, n, what, float((ring - one_step).abs().max()))

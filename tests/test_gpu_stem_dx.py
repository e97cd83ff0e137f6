"""GPU: the input gradient of the residual stem (node_stem_bwd_dx; csrc/kernels_stem.hip: k_stem_conv0_dgrad).  The transposed
first layer alone against an fp64 `conv_transpose2d`, then the whole stem's image gradient through the opt-in
`ResidualStem.input_grad` against the same modules run in fp64 on the CPU -- with the bounds the existing stem tests use for
the same kernel family (tests/test_gpu_stem.py: 1e-5 for one convolution, 2e-5 / 5e-5 for whole-stem gradients)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_stem import _stem_pair

pytestmark = pytest.mark.gpu


def _conv0_dgrad(n, in_ch, h, w, w0, dy):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeStemShape(n, in_ch, h, w, 64, 1e-5)
    nbytes = lib.node_stem_conv0_dgrad_workspace_bytes(C.byref(shape))
    assert nbytes > 0, lib.node_last_error()
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    res = torch.full((n, in_ch, h, w), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.node_stem_conv0_dgrad(C.byref(shape), w0.data_ptr(), dy.data_ptr(), res.data_ptr(), (ws.data_ptr() + 255) & ~255, nbytes,
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return res.cpu()


@pytest.mark.parametrize('geom', [(1, 28, 28), (3, 28, 28), (1, 32, 32), (3, 32, 32), (3, 7, 9), (2, 9, 7), (3, 17, 67)],
                         ids=lambda g: 'in%d_%dx%d' % g)
@pytest.mark.parametrize('n', [1, 3])
def test_conv0_dgrad_matches_fp64(geom, n):
    """Sides 28 and 32 (one tile column, 4 tile rows of 8 with a ragged last one at 28), 7 x 9 / 9 x 7 (a single ragged tile: every
    pixel within two of a border), 17 x 67 (three tile columns: the halo across a column seam)."""
    in_ch, h, w = geom
    gen = torch.Generator().manual_seed(in_ch + h + w + n)
    w0 = torch.randn(64, in_ch, 3, 3, generator=gen) / (9 * in_ch) ** 0.5
    dy = torch.randn(n, 64, h - 2, w - 2, generator=gen)
    ref = F.conv_transpose2d(dy.double(), w0.double())
    assert ref.shape == (n, in_ch, h, w)
    got = _conv0_dgrad(n, in_ch, h, w, w0.cuda(), dy.cuda())
    assert bool(torch.isfinite(got).all())          # every element written
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print('conv0 dgrad %s n %d: max error / max|ref| = %.2e' % (geom, n, err))
    assert err <= 1e-5, (geom, n, err)
    again = _conv0_dgrad(n, in_ch, h, w, w0.cuda(), dy.cuda())
    assert torch.equal(got, again)                  # no atomics: the same bits on every run


def _grads(stem):
    return {name: p.grad.detach().clone() for name, p in stem.named_parameters()}


@pytest.mark.parametrize('case,w4', [((3, 32, 64, 2), 1), ((1, 28, 64, 3), 1), ((3, 32, 256, 8), 1), ((3, 32, 256, 8), 0)],
                         ids=['in3_32px_f64_n2', 'in1_28px_f64_n3', 'in3_32px_f256_n8_w4', 'in3_32px_f256_n8_gather'])
def test_stem_input_gradient_through_the_opt_in(case, w4, monkeypatch):
    in_ch, side, filters, n = case
    takes_w4 = w4 == 1 and side == 32 and n % 8 == 0 and filters % 128 == 0
    monkeypatch.setenv('NODE_TUNE_STEM_W4', str(w4))
    stem, ref = _stem_pair(in_ch, filters, seed=in_ch + filters)
    stem = stem.cuda()
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(n, in_ch, side, side, generator=gen)
    xd = x.double().requires_grad_(True)
    out_ref = ref(xd)
    cot = torch.randn(out_ref.shape, generator=gen)
    out_ref.backward(cot.double())

    # the opt-in off: the module sequence, as ever
    xg = x.cuda().requires_grad_(True)
    assert type(stem(xg).grad_fn).__name__ != '_StemFnBackward'

    stem.input_grad = True
    # 1. frozen parameters: grads = NULL, the data-gradient chain alone
    for p in stem.parameters():
        p.requires_grad_(False)
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == '_StemFnBackward'
    out.backward(cot.cuda())
    dx_frozen = xg.grad.detach().clone()
    assert all(p.grad is None for p in stem.parameters())
    err = float((dx_frozen.cpu().double() - xd.grad).abs().max() / xd.grad.abs().max())
    print('stem %s (w4 %s): input gradient max error / max|ref| = %.2e' % (case, takes_w4, err))
    assert err <= (5e-5 if takes_w4 else 2e-5), err

    # 2. parameters with gradients: d_x the same bits, the sixteen parameter gradients node_stem_bwd's bits
    for p in stem.parameters():
        p.requires_grad_(True)
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == '_StemFnBackward'
    out.backward(cot.cuda())
    assert torch.equal(xg.grad, dx_frozen)
    with_dx = _grads(stem)
    assert len(with_dx) == 16
    stem.zero_grad(set_to_none=True)
    out = stem(x.cuda())                                 # no input gradient: node_stem_bwd
    assert type(out.grad_fn).__name__ == '_StemFnBackward'
    out.backward(cot.cuda())
    plain = _grads(stem)
    for name in plain:
        assert torch.equal(with_dx[name], plain[name]), name

    # the opt-in off again: the module sequence
    stem.input_grad = False
    assert type(stem(x.cuda().requires_grad_(True)).grad_fn).__name__ != '_StemFnBackward'


def test_stem_with_input_gradient_runs_no_library_convolution():
    """Forward + input-gradient backward of the opted-in stem: PyTorch dispatches no convolution, GroupNorm, transpose or ReLU."""
    from torch.profiler import ProfilerActivity, profile
    stem, _ = _stem_pair(3, 256, seed=7)
    stem = stem.cuda()
    stem.input_grad = True
    for p in stem.parameters():
        p.requires_grad_(False)
    x = torch.randn(8, 3, 32, 32).cuda()
    xg = x.clone().requires_grad_(True)
    stem(xg).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        xg = x.clone().requires_grad_(True)
        out = stem(xg)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('conv', 'miopen', 'group_norm', 'native_group_norm', 'transpose', 'relu'))]
    assert not bad, bad
    assert any('_StemFn' in k for k in names), names


def test_bwd_dx_refuses_a_missing_output():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeStemShape(2, 3, 32, 32, 64, 1e-5)
    t = torch.zeros(16, device='cuda')
    ps = _lib.NodeStemParams(*[t.data_ptr()] * 16)
    rc = lib.node_stem_bwd_dx(C.byref(shape), C.byref(ps), t.data_ptr(), t.data_ptr(), None, None, t.data_ptr(), 1 << 20, None)
    assert rc == -1, lib.node_last_error()

"""GPU: the `convolution` stem (model.py:148-164, `ConvDownsample`) as one node of the library
(neural_ode_features_amd/convstem.py, csrc/convstem_api.hip on the kernels of csrc/kernels_stem.hip): output and all ten
parameter gradients against the same modules in fp64 on the CPU and against the reference's own stem
(tests/golden/stem_convolution_c64.pt), bit-reproducibility, the dispatcher trace, and the shapes that keep the module
sequence."""
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _stem_pair(in_ch, filters, seed, kink_free=False):
    """tests/test_gpu_stem.py::_stem_pair for the `convolution` stem (its GroupNorms are children 1 and 4)"""
    import neural_ode_features_amd as nof
    torch.manual_seed(seed)
    net = nof.ODENet(in_ch, out=10, n_filters=filters, downsample='convolution', adjoint=True)
    stem = net.downsample.module
    assert isinstance(stem, nof.ConvStem)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in (1, 4):
            for p in (stem[i].weight, stem[i].bias):
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
            if kink_free:
                stem[i].bias.add_(8.0)          # every pre-activation positive: no ReLU mask can differ between fp32 and fp64
    return stem, copy.deepcopy(stem).double()


def _rel(a, b):
    return float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max())


def _run(case, fused=True):
    in_ch, side, filters, n = case[:4]
    stem, ref = _stem_pair(in_ch, filters, seed=in_ch + filters, kink_free=len(case) > 4 and case[4])
    stem = stem.cuda()
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(n, in_ch, side, side, generator=gen)
    out = stem(x.cuda())
    assert (type(out.grad_fn).__name__ == '_ConvStemFnBackward') == fused          # the fused node / the module sequence
    out_ref = ref(x.double())
    assert out.shape == out_ref.shape
    cot = torch.randn(out_ref.shape, generator=gen)
    out.backward(cot.cuda())
    out_ref.backward(cot.double())
    errs = {'out': _rel(out, out_ref)}
    for (name, p), (_, q) in zip(stem.named_parameters(), ref.named_parameters()):
        errs[name] = _rel(p.grad, q.grad) if fused else float((p.grad.cpu().double() - q.grad).norm() / q.grad.norm())
    return errs, [out.detach().clone()] + [p.grad.clone() for p in stem.parameters()]


@pytest.mark.parametrize('case', [(3, 32, 256, 6, False), (1, 28, 64, 5, True), (3, 32, 64, 8, False)],
                         ids=lambda c: 'in%d_%dpx_f%d_n%d%s' % (c[:4] + ('_kinkfree' if c[4] else '',)))
def test_convstem_forward_and_every_gradient_match_fp64(case):
    """Max-norm parity of the output and of all ten parameter gradients with the fp64 run at the whole-stem bounds of
    tests/test_gpu_stem.py (2e-5 of the largest entry), and two runs that agree bit for bit in every output.

    The MNIST case runs on kink-free parameters (GroupNorm biases at +8, tests/test_gpu_stem.py's rule): with this seed's
    ordinary parameters ONE of its 54 080 pre-activations behind the second GroupNorm is 6.1e-8 in fp64, which fp32 rounding
    turns negative -- PyTorch's own fp32 modules on the CPU give -3.5e-8 -- so its ReLU mask differs from the fp64 run's and
    that single element moves the gradients of every layer in front of the last convolution by 2e-3 .. 1.2e-2 (measured on
    the fused path: output 1.0e-6, `6.weight` 6.7e-7, `6.bias` 1.5e-7, `3.weight` 1.2e-2).  The other two cases have no
    pre-activation within 1.6e-6 of zero and hold the bound on ordinary parameters."""
    errs, first = _run(case)
    for k, e in errs.items():
        print('conv stem %s: %-10s max error / max|ref| = %.2e' % (case, k, e))
    _, second = _run(case)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert max(errs.values()) <= 2e-5, errs


def test_convstem_matches_the_reference_fixture(golden_dir):
    """tests/golden/stem_convolution_c64.pt (+ _grads.pt): the reference's own `ConvDownsample(1, 64)` (model.py:148-164,
    imported by tests/golden/make_golden_convstem.py) on a [2, 1, 28, 28] input -- output and every parameter gradient.  The
    reference's state_dict loads unchanged (same keys)."""
    import neural_ode_features_amd as nof
    g = torch.load(os.path.join(golden_dir, 'stem_convolution_c64.pt'), map_location='cpu', weights_only=False)
    grads = torch.load(os.path.join(golden_dir, 'stem_convolution_c64_grads.pt'), map_location='cpu', weights_only=False)['grads']
    net = nof.ODENet(1, out=10, n_filters=64, downsample='convolution', adjoint=True)
    stem = net.downsample           # (the wrapper holds the body under `.module`, like the reference's ConvDownsample)
    stem.load_state_dict(g['state_dict'])
    stem = stem.cuda()
    out = stem(g['x'].cuda())
    assert type(out.grad_fn).__name__ == '_ConvStemFnBackward'
    out.backward(g['cot'].cuda())
    err = float((out.detach().cpu() - g['out']).abs().max() / g['out'].abs().max())
    print('reference conv stem fixture: output max error / max|ref| = %.2e' % err)
    assert err <= 2e-5
    assert sorted(grads) == sorted(k for k, _ in stem.named_parameters())
    for name, p in stem.named_parameters():
        e = float((p.grad.cpu() - grads[name]).abs().max() / grads[name].abs().max())
        print('  grad %-18s %.2e' % (name, e))
        assert e <= 1e-4, (name, e)       # (the fixture itself is fp32: PyTorch-CPU's own rounding sits at ~1e-6)


def test_convstem_runs_no_library_convolution():
    """ONE autograd node whose forward and backward are calls into libnode_hip.so: the dispatcher trace of a forward + backward
    holds no convolution, GroupNorm, ReLU or transpose operator (the check of test_stem_runs_no_library_convolution)."""
    from torch.profiler import ProfilerActivity, profile
    stem, _ = _stem_pair(3, 256, seed=7)
    stem = stem.cuda()
    x = torch.randn(8, 3, 32, 32).cuda()
    stem(x).sum().backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        out = stem(x)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [k for k in names if any(s in k.lower() for s in ('conv', 'miopen', 'group_norm', 'native_group_norm', 'transpose', 'relu'))
           and '_ConvStemFn' not in k]
    assert not bad, bad
    assert any('_ConvStemFn' in k for k in names), names


@pytest.mark.parametrize('case', [(3, 32, 192, 4), (3, 64, 64, 2)], ids=['filters192', '64px'])
def test_shapes_the_kernels_refuse_run_the_module_sequence(case):
    """filters = 192 (no power of two) and a 64x64 input (its 62x62 image does not fit the GroupNorm passes' LDS block) are
    refused by the library with a message, run `nn.Sequential.forward` and still match fp64: the output to 1e-4 of its largest
    entry (PyTorch's fp32 convolutions), the gradients to 1e-2 in relative L2 -- a 64x64 input has 250 k pre-activations per
    sample, one of which may land within fp32 rounding of zero; its flipped ReLU mask moves one GroupNorm-bias entry (a sum
    over 3844 pixels of random sign) by ~2e-2 and that tensor's L2 norm by ~2e-3, while a wiring mistake moves it by O(1)."""
    import ctypes as C
    from neural_ode_features_amd import _lib
    in_ch, side, filters, n = case
    lib = _lib.load()
    assert lib.node_convstem_workspace_bytes(C.byref(_lib.NodeConvStemShape(n, in_ch, side, side, filters, 1e-5)), 1) == 0
    assert ('filters' if filters == 192 else 'LDS') in lib.node_last_error().decode()
    errs, _ = _run(case, fused=False)
    print('conv stem %s on the module sequence: worst error %.2e' % (case, max(errs.values())))
    assert errs['out'] <= 1e-4 and max(errs.values()) <= 1e-2, errs


def test_convstem_input_gradient_and_second_backward():
    """An input that requires a gradient (saliency maps, adversarial examples) takes the module sequence and gets its gradient;
    a second backward through one fused forward raises instead of crashing; a forward under no_grad stays fused."""
    stem, ref = _stem_pair(3, 64, seed=3)
    stem = stem.cuda()
    x = torch.randn(2, 3, 32, 32)
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ != '_ConvStemFnBackward'
    out.sum().backward()
    xd = x.double().requires_grad_(True)
    ref(xd).sum().backward()
    assert float((xg.grad.cpu().double() - xd.grad).abs().max() / xd.grad.abs().max()) <= 1e-3
    out = stem(x.cuda())
    assert type(out.grad_fn).__name__ == '_ConvStemFnBackward'
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        out.sum().backward()
    with torch.no_grad():
        quiet = stem(x.cuda())
    assert quiet.grad_fn is None and torch.equal(quiet, out.detach())

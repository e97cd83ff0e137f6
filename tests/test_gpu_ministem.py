"""GPU: the `minimal` stem (model.py:129-145, `MinimalConvDownsample`) as one node of the library
(neural_ode_features_amd/ministem.py, csrc/ministem_api.hip on the kernels of csrc/kernels_ministem.hip) and the input
gradient of the `convolution` stem (node_convstem_bwd_dx): output, all ten parameter gradients and the image's gradient
against the same modules in fp64 on the CPU and against the reference's own stem (tests/golden/stem_minimal_c64.pt),
bit-reproducibility, the `input_grad` switch with its NULL arguments, the dispatcher trace, and the shapes that keep the
module sequence."""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

VANISHING = ('0.bias', '3.bias')      # biases in front of a GroupNorm with one channel per group: zero gradient in exact arithmetic


def _pair(in_ch, filters, seed, kink_free=False, downsample='minimal'):
    """tests/test_gpu_convstem.py::_stem_pair with the `minimal` stem (its GroupNorms are children 1 and 4)"""
    import neural_ode_features_amd as nof
    torch.manual_seed(seed)
    net = nof.ODENet(in_ch, out=10, n_filters=filters, downsample=downsample, adjoint=True)
    stem = net.downsample.module
    assert isinstance(stem, nof.MinimalStem if downsample == 'minimal' else nof.ConvStem)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in (1, 4):
            for p in (stem[i].weight, stem[i].bias):
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
            if kink_free:
                stem[i].bias.add_(8.0)          # every pre-activation positive: no ReLU mask can differ between fp32 and fp64
    return stem, copy.deepcopy(stem).double()


def _fp64_run(ref, x, cot):
    """Output, input gradient, parameter gradients and, per vanishing bias, max_c sum_{n,p} |dh[n, c, p]| of the gradient dh at
    that convolution's output (a backward hook on the fp64 modules)."""
    for p in ref.parameters():
        p.grad = None
    dh = {}
    xd = x.double().requires_grad_(True)
    t = xd
    for i, m in enumerate(ref):
        t = m(t)
        if i in (0, 3):
            t.register_hook(lambda g, i=i: dh.__setitem__('%d.bias' % i, float(g.abs().sum(dim=(0, 2, 3)).max())))
    t.backward(cot.double())
    return t.detach(), xd.grad.clone(), {k: p.grad.clone() for k, p in ref.named_parameters()}, dh


@functools.lru_cache(maxsize=None)
def _reference(case, kink_free=False):
    """The fp64 run of a case (in_ch, h, w, filters, n) on the CPU: computed once, shared, never modified."""
    in_ch, h, w, filters, n = case
    _, ref = _pair(in_ch, filters, in_ch + filters, kink_free)
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(n, in_ch, h, w, generator=gen)
    out_shape = ref(x.double()).shape
    cot = torch.randn(out_shape, generator=gen)
    return (x, cot) + _fp64_run(ref, x, cot)


def _rel(a, b):
    return float((a.detach().cpu().double() - b).abs().max() / b.abs().max())


def _fused_run(case, kink_free=False):
    in_ch, h, w, filters, n = case
    x, cot = _reference(case, kink_free)[:2]
    stem, _ = _pair(in_ch, filters, in_ch + filters, kink_free)
    stem = stem.cuda()
    stem.input_grad = True
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == '_MiniStemFnBackward'
    out.backward(cot.cuda())
    return out.detach().clone(), xg.grad.clone(), {k: p.grad.clone() for k, p in stem.named_parameters()}


CASES = [(3, 32, 32, 256, 6), (1, 28, 28, 64, 5), (3, 32, 32, 64, 8), (3, 14, 22, 64, 3), (3, 10, 10, 64, 2)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'in%d_%dx%d_f%d_n%d' % c)
def test_ministem_forward_and_every_gradient_match_fp64(case):
    """Max-norm parity of the output, of the image's gradient (`input_grad` on) and of eight of the ten parameter gradients
    with the fp64 run at the project's whole-stem bound (2e-5 of the largest entry), on ordinary parameters; `0.bias` and
    `3.bias` -- zero in exact arithmetic, one channel per group -- absolutely: max|grad| <= 2e-5 x max_c sum_{n,p} |dh| with dh
    the fp64 gradient at that convolution's output.  Two runs agree bit for bit in every output."""
    _, _, out_ref, dx_ref, grads_ref, dh = _reference(case)
    out, dx, grads = _fused_run(case)
    errs = {'out': _rel(out, out_ref), 'd_x': _rel(dx, dx_ref)}
    for k, g in grads.items():
        if k in VANISHING:
            errs[k] = float(g.abs().max()) / dh[k]
        else:
            errs[k] = _rel(g, grads_ref[k])
    for k, e in errs.items():
        print('minimal stem %s: %-10s %s = %.2e' % (case, k, 'max|grad| / max_c sum|dh|' if k in VANISHING else 'max error / max|ref|', e))
    out2, dx2, grads2 = _fused_run(case)
    assert torch.equal(out, out2) and torch.equal(dx, dx2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    assert sorted(grads) == sorted(grads_ref) and len(grads) == 10
    assert max(errs.values()) <= 2e-5, errs


def _grads(stem):
    return {k: p.grad.detach().clone() for k, p in stem.named_parameters()}


@pytest.mark.parametrize('kind,case', [('minimal', (3, 32, 32, 64, 2)), ('convolution', (3, 32, 32, 64, 2)), ('convolution', (1, 28, 28, 64, 3))],
                         ids=['minimal_cifar', 'convolution_cifar', 'convolution_mnist'])
def test_input_gradient_through_the_opt_in(kind, case):
    """tests/test_gpu_stem_dx.py::test_stem_input_gradient_through_the_opt_in for `MinimalStem` and `ConvStem`: the switch off
    keeps the module sequence; on, frozen parameters run the data-gradient chain alone (grads = NULL) with d_x within 2e-5 of
    fp64; unfrozen, d_x is the same bits and every parameter gradient the bits of the backward without an input gradient."""
    in_ch, h, w, filters, n = case
    node = '_MiniStemFnBackward' if kind == 'minimal' else '_ConvStemFnBackward'
    stem, ref = _pair(in_ch, filters, in_ch + filters, downsample=kind)
    stem = stem.cuda()
    gen = torch.Generator().manual_seed(99)
    x = torch.randn(n, in_ch, h, w, generator=gen)
    xd = x.double().requires_grad_(True)
    out_ref = ref(xd)
    cot = torch.randn(out_ref.shape, generator=gen)
    out_ref.backward(cot.double())

    # the opt-in off: the module sequence
    assert stem.input_grad is False
    assert type(stem(x.cuda().requires_grad_(True)).grad_fn).__name__ != node

    stem.input_grad = True
    # 1. frozen parameters: grads = NULL, the data-gradient chain alone
    for p in stem.parameters():
        p.requires_grad_(False)
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == node
    out.backward(cot.cuda())
    dx_frozen = xg.grad.detach().clone()
    assert all(p.grad is None for p in stem.parameters())
    err = float((dx_frozen.cpu().double() - xd.grad).abs().max() / xd.grad.abs().max())
    print('%s stem %s: input gradient max error / max|ref| = %.2e' % (kind, case, err))
    assert err <= 2e-5, err

    # 2. parameters with gradients: d_x the same bits, the ten parameter gradients the bits of the backward without d_x
    for p in stem.parameters():
        p.requires_grad_(True)
    xg = x.cuda().requires_grad_(True)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == node
    out.backward(cot.cuda())
    assert torch.equal(xg.grad, dx_frozen)
    with_dx = _grads(stem)
    assert len(with_dx) == 10
    stem.zero_grad(set_to_none=True)
    out = stem(x.cuda())                                 # no input gradient
    assert type(out.grad_fn).__name__ == node
    out.backward(cot.cuda())
    plain = _grads(stem)
    for name in plain:
        assert torch.equal(with_dx[name], plain[name]), name

    # the opt-in off again: the module sequence
    stem.input_grad = False
    assert type(stem(x.cuda().requires_grad_(True)).grad_fn).__name__ != node


def test_null_arguments_of_the_backward():
    """node_ministem_bwd with grads and d_x both NULL, and node_convstem_bwd_dx without d_x: NODE_ERR_NULL, nothing launched."""
    import ctypes as C
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    x = torch.randn(2, 3, 32, 32).cuda()
    g = torch.randn(2, 64, 7, 7).cuda()
    for kind, S, P, size, bwd in (('minimal', _lib.NodeMiniStemShape, _lib.NodeMiniStemParams, lib.node_ministem_workspace_bytes, lib.node_ministem_bwd),
                                  ('convolution', _lib.NodeConvStemShape, _lib.NodeConvStemParams, lib.node_convstem_workspace_bytes, lib.node_convstem_bwd_dx)):
        stem, _ = _pair(3, 64, 5, downsample=kind)
        stem = stem.cuda()
        ps = _lib_params(P, stem)
        sh = S(2, 3, 32, 32, 64, 1e-5)
        nbytes = size(C.byref(sh), 1)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
        wsp = (ws.data_ptr() + 255) & ~255
        assert bwd(C.byref(sh), C.byref(ps), x.data_ptr(), g.data_ptr(), None, None, wsp, nbytes, None) == -1, kind
        assert b'NULL' in lib.node_last_error()
    torch.cuda.synchronize()


def _lib_params(P, stem):
    return P(*[p.data_ptr() for p in stem.parameters()])


def test_ministem_matches_the_reference_fixture(golden_dir):
    """tests/golden/stem_minimal_c64.pt: the reference's own `MinimalConvDownsample(1, 64)` (model.py:129-145, imported by
    tests/golden/make_golden_ministem.py) on a [2, 1, 28, 28] input -- output within 2e-5, every parameter gradient within 1e-4
    of max|ref| (the fixture is fp32); the two vanishing biases absolutely, against 2e-5 x max_c sum |dh| from an fp64 rerun of
    the loaded modules on the CPU.  The reference's state_dict loads unchanged (same keys)."""
    import neural_ode_features_amd as nof
    g = torch.load(os.path.join(golden_dir, 'stem_minimal_c64.pt'), map_location='cpu', weights_only=False)
    net = nof.ODENet(1, out=10, n_filters=64, downsample='minimal', adjoint=True)
    stem = net.downsample           # (the wrapper holds the body under `.module`, like the reference's MinimalConvDownsample)
    stem.load_state_dict(g['state_dict'])
    _, _, _, dh = _fp64_run(copy.deepcopy(stem.module).double(), g['x'], g['cot'])
    stem = stem.cuda()
    out = stem(g['x'].cuda())
    assert type(out.grad_fn).__name__ == '_MiniStemFnBackward'
    out.backward(g['cot'].cuda())
    err = float((out.detach().cpu() - g['out']).abs().max() / g['out'].abs().max())
    print('reference minimal stem fixture: output max error / max|ref| = %.2e' % err)
    assert err <= 2e-5
    assert sorted(g['grads']) == sorted(k for k, _ in stem.named_parameters())
    for name, p in stem.named_parameters():
        short = name[len('module.'):]
        if short in VANISHING:
            e = float(p.grad.abs().max()) / dh[short]
            print('  grad %-18s max|grad| / max_c sum|dh| = %.2e' % (name, e))
            assert e <= 2e-5, (name, e)
        else:
            e = float((p.grad.cpu() - g['grads'][name]).abs().max() / g['grads'][name].abs().max())
            print('  grad %-18s %.2e' % (name, e))
            assert e <= 1e-4, (name, e)


def _dispatched(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


def _library_ops(names, own):
    return [k for k in names if any(s in k.lower() for s in ('conv', 'miopen', 'group_norm', 'transpose', 'relu'))
            and not any(o in k for o in own)]


def test_ministem_runs_no_library_convolution():
    """ONE autograd node whose forward and backward are calls into libnode_hip.so: the dispatcher trace of a forward + backward
    holds no convolution, GroupNorm, ReLU or transpose operator."""
    stem, _ = _pair(3, 256, seed=7)
    stem = stem.cuda()
    x = torch.randn(8, 3, 32, 32).cuda()

    def step():
        out = stem(x)
        out.backward(torch.ones_like(out))
    names = _dispatched(step)
    assert not _library_ops(names, ('_MiniStemFn',)), names
    assert any('_MiniStemFn' in k for k in names), names


def test_resnet_on_the_minimal_stem_runs_no_library_convolution():
    """`ResNet(3, n_filters=64, downsample='minimal')` at [8, 3, 32, 32]: stem, trunk and head, forward + backward."""
    import neural_ode_features_amd as nof
    torch.manual_seed(11)
    net = nof.ResNet(3, n_filters=64, downsample='minimal').cuda()
    x = torch.randn(8, 3, 32, 32).cuda()

    def step():
        net(x).sum().backward()
    names = _dispatched(step)
    assert not _library_ops(names, ('_MiniStemFn', '_TrunkFn')), names
    assert any('_MiniStemFn' in k for k in names) and any('_TrunkFn' in k for k in names), names


def test_opted_in_convstem_runs_no_library_convolution():
    """Forward + input-gradient backward of an opted-in `ConvStem` with frozen parameters."""
    stem, _ = _pair(3, 256, seed=7, downsample='convolution')
    stem = stem.cuda()
    stem.input_grad = True
    for p in stem.parameters():
        p.requires_grad_(False)
    x = torch.randn(8, 3, 32, 32).cuda()

    def step():
        xg = x.clone().requires_grad_(True)
        out = stem(xg)
        out.backward(torch.ones_like(out))
        assert xg.grad is not None
    names = _dispatched(step)
    assert not _library_ops(names, ('_ConvStemFn',)), names
    assert any('_ConvStemFn' in k for k in names), names


@pytest.mark.parametrize('kind,node', [('minimal', '_MiniStemFn'), ('convolution', '_ConvStemFn')])
def test_bim_goes_through_the_fused_stem(kind, node):
    """`attack.bim` on a ResNet with the `minimal` / `convolution` stem, n = 2, two L-infinity iterations: the stem's fused node
    runs with its input gradient (no convolution or GroupNorm of PyTorch's library is dispatched), the result stays inside the
    ball and the bounds, and the stem's `input_grad` switch and the parameters' `requires_grad` are as before afterwards."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd.attack import bim
    torch.manual_seed(3)
    net = nof.ResNet(3, out=10, n_filters=64, downsample=kind).eval().cuda()
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        labels = net(x.cuda()).argmax(1)
    found = {}

    def attack():
        found['r'] = bim(net, x.cuda(), labels, norm=float('inf'), epsilon=.03, stepsize=.01, iterations=2)
    names = _dispatched(attack)
    assert any(node in k for k in names), names
    bad = [k for k in names if any(s in k.lower() for s in ('conv', 'miopen', 'group_norm')) and node not in k]
    assert not bad, bad
    d = (found['r'].adversarial.cpu() - x).abs()
    assert 0 < float(d.max()) <= .02 + 1e-6
    assert float(found['r'].adversarial.min()) >= 0.0 and float(found['r'].adversarial.max()) <= 1.0
    assert net.downsample.module.input_grad is False and all(p.requires_grad for p in net.parameters())


def test_filters_the_kernels_refuse_run_the_module_sequence():
    """filters = 192 (no power of two) is refused by the library with a message naming the limit, runs `nn.Sequential.forward`
    and still matches fp64 to 1e-4 of the output's largest entry.  (The kernels hold no plane in LDS: no image is too large.)"""
    import ctypes as C
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    assert lib.node_ministem_workspace_bytes(C.byref(_lib.NodeMiniStemShape(4, 3, 32, 32, 192, 1e-5)), 1) == 0
    assert 'filters' in lib.node_last_error().decode() and 'power of two' in lib.node_last_error().decode()
    stem, ref = _pair(3, 192, seed=3 + 192)
    stem = stem.cuda()
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(99))
    out = stem(x.cuda())
    assert type(out.grad_fn).__name__ != '_MiniStemFnBackward'
    assert _rel(out, ref(x.double()).detach()) <= 1e-4


def test_second_backward_and_no_grad():
    """A second backward through one fused forward raises instead of crashing; a forward under no_grad stays fused."""
    stem, _ = _pair(3, 64, seed=3)
    stem = stem.cuda()
    x = torch.randn(2, 3, 32, 32).cuda()
    out = stem(x)
    assert type(out.grad_fn).__name__ == '_MiniStemFnBackward'
    out.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        out.sum().backward()
    with torch.no_grad():
        quiet = stem(x)
    assert quiet.grad_fn is None and torch.equal(quiet, out.detach())

"""GPU: the banded residual stem (node_stem_banded_fwd / node_stem_banded_bwd / node_stem_banded_bwd_dx, csrc/kernels_stem_banded.hip;
`stem._BandedStemFn`) on images past the resident GroupNorm passes' 2400 pixels, against the float64 module sequence on the CPU.

Bounds: the project's own for the stem (tests/test_gpu_stem.py) -- output <= 2e-5 of max |ref|, every gradient <= 2e-5 of its
largest entry, in max norm -- on kink-free parameters (norm biases + 8: no ReLU mask can differ between two precisions) and, with
ordinary parameters, under the recorded seed of tests/stem_banded_cases.py (the seed rule; asserted by tests/test_stem_banded_host.py).
The fp32 module sequence on a CPU measured <= 5.0e-7 on the output and <= 6.4e-6 on the worst gradient against fp64 at these shapes."""
import copy
import ctypes as C

import pytest
import torch

from tests import stem_banded_cases as B
from tests.helpers import tune_env

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _on_gpu(stem_cpu):
    stem = copy.deepcopy(stem_cpu).cuda()
    stem.fused_banded = True          # (explicitly: these tests do not depend on the shipped default)
    return stem


def _module_run(name, kink_free, input_grad=True, frozen=False):
    """The stem through ResidualStem.forward on the GPU: {'out', 'grad00' ... 'grad15' in the library's order, 'dx'} as float64 on the CPU"""
    from neural_ode_features_amd import stem as S
    mod, x, cot = B.reference(name, kink_free)['inputs']
    stem = _on_gpu(mod)
    stem.input_grad = input_grad
    if frozen:
        for p in stem.parameters():
            p.requires_grad_(False)
    xg = x.cuda().requires_grad_(input_grad)
    out = stem(xg)
    assert type(out.grad_fn).__name__ == '_BandedStemFnBackward', type(out.grad_fn).__name__
    out.backward(cot.cuda())
    torch.cuda.synchronize()
    res = {'out': out.detach().cpu().double()}
    if not frozen:
        for i, p in enumerate(S._params_of(stem)):
            res['grad%02d' % i] = p.grad.detach().cpu().double()
    if input_grad:
        res['dx'] = xg.grad.detach().cpu().double()
    return res


def _abi_run(prefix, name, kink_free):
    """The same through the C ABI (`prefix`_fwd, `prefix`_bwd_dx): what the Python gate would not send to this family"""
    from neural_ode_features_amd import _lib
    from neural_ode_features_amd import stem as S
    lib = _lib.load()
    mod, x, cot = B.reference(name, kink_free)['inputs']
    n, in_ch, h, w, filters = B.SHAPES[name]
    shape = _lib.NodeStemShape(n, in_ch, h, w, filters, float(mod[1].norm1.eps))
    ps = [p.detach().cuda().contiguous() for p in S._params_of(mod)]
    grads = [torch.full_like(p, float('nan')) for p in ps]
    xg, cg = x.cuda().contiguous(), cot.cuda().contiguous()
    nbytes = getattr(lib, prefix + '_workspace_bytes')(C.byref(shape))
    assert nbytes > 0, _lib.last_error() if hasattr(_lib, 'last_error') else nbytes
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    wsp = (ws.data_ptr() + 255) // 256 * 256
    out = torch.full(tuple(cot.shape), float('nan'), device='cuda')
    dx = torch.full_like(xg, float('nan'))
    st = torch.cuda.current_stream().cuda_stream
    struct = lambda ts: _lib.NodeStemParams(*[t.data_ptr() for t in ts])
    _lib.check(getattr(lib, prefix + '_fwd')(C.byref(shape), C.byref(struct(ps)), xg.data_ptr(), out.data_ptr(), wsp, nbytes, st))
    _lib.check(getattr(lib, prefix + '_bwd_dx')(C.byref(shape), C.byref(struct(ps)), xg.data_ptr(), cg.data_ptr(), C.byref(struct(grads)),
                                                dx.data_ptr(), wsp, nbytes, st))
    torch.cuda.synchronize()
    res = {'out': out.cpu().double(), 'dx': dx.cpu().double()}
    for i, g in enumerate(grads):
        res['grad%02d' % i] = g.cpu().double()
    return res


def _errors(got, ref):
    """max-norm error of every result relative to the largest entry of its reference"""
    errs = {}
    for k, v in got.items():
        r = ref[k]
        assert v.shape == r.shape, (k, v.shape, r.shape)
        assert bool(torch.isfinite(v).all()), k + ' has non-finite entries (an element never written?)'
        errs[k] = float((v - r).abs().max() / r.abs().max())
    return errs


def _assert_parity(what, got, ref, relative_l2=False):
    errs = _errors(got, ref)
    worst = max((k for k in errs if k != 'out'), key=errs.get)
    print('%s: output %.2e, worst gradient %s %.2e' % (what, errs['out'], worst, errs[worst]))
    assert len(errs) == 18, sorted(errs)              # the output, sixteen parameter gradients, the image's gradient
    if relative_l2:      # (B.RELATIVE_L2, ordinary parameters: a flipped ReLU mask moves one element by O(1))
        l2 = {k: float((got[k] - ref[k]).norm() / ref[k].norm()) for k in got if k != 'out'}
        print('%s: worst relative L2 of a gradient %.2e' % (what, max(l2.values())))
        bad = {k: e for k, e in l2.items() if not e <= 2e-2}
        assert errs['out'] <= TOL and not bad, (what, errs['out'], bad)
        return
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, (what, bad)


@pytest.mark.parametrize('kink_free', [True, False], ids=['kinkfree', 'recorded_seed'])
@pytest.mark.parametrize('name', B.GATE)
def test_output_every_gradient_and_the_image_gradient_match_fp64(name, kink_free):
    n, in_ch, h, w, filters = B.SHAPES[name]
    assert (h - 2) * (w - 2) > 2400                    # past the resident node: the gate sends it to _BandedStemFn
    got = _module_run(name, kink_free)
    _assert_parity('%s %s' % (name, 'kink-free' if kink_free else 'seed %d' % B.SEEDS[name]), got, B.reference(name, kink_free)['ref'],
                   relative_l2=not kink_free and name in B.RELATIVE_L2)


@pytest.mark.parametrize('kink_free', [True, False], ids=['kinkfree', 'recorded_seed'])
@pytest.mark.parametrize('name', B.ABI_ONLY)
def test_every_norm_banded_in_many_bands_matches_fp64(name, kink_free):
    """NODE_TUNE_STEM_BANDED=all with 16-pixel bands through the ABI: all four norms banded (2 and 8 channels per group), tens of bands,
    a short last one.  The resident node's error at the same shape is printed next to it."""
    from neural_ode_features_amd import _lib
    n, in_ch, h, w, filters = B.SHAPES[name]
    ref = B.reference(name, kink_free)['ref']
    with tune_env(**B.ALL_ENV):
        plan = _lib.stem_banded_plan(n, in_ch, h, w, filters)
        assert all(g['banded'] and g['band_px'] == 16 for g in plan['gn']) and not plan['takes_w4'], plan
        assert any(g['hw'] % 16 for g in plan['gn'])              # a short last band
        got = _abi_run('node_stem_banded', name, kink_free)
    resident = _errors(_abi_run('node_stem', name, kink_free), ref)
    worst = max((k for k in resident if k != 'out'), key=resident.get)
    print('%s resident node: output %.2e, worst gradient %s %.2e' % (name, resident['out'], worst, resident[worst]))
    _assert_parity('%s banded %s' % (name, 'kink-free' if kink_free else 'seed %d' % B.SEEDS[name]), got, ref)


def _kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


def test_backward_variants_agree_and_frozen_parameters_run_the_data_gradient_chain_alone():
    name = 's64_f128'
    ref = B.reference(name, True)['ref']
    params_only = _module_run(name, True, input_grad=False)
    full = _module_run(name, True, input_grad=True)
    frozen = _module_run(name, True, input_grad=True, frozen=True)
    assert 'dx' not in params_only and len(params_only) == 17 and len(frozen) == 2
    errs = _errors(params_only, ref)
    assert max(errs.values()) <= TOL, errs
    for k, v in params_only.items():                       # node_stem_banded_bwd and node_stem_banded_bwd_dx: the same parameter gradients
        assert torch.equal(v, full[k]), k
    assert torch.equal(frozen['dx'], full['dx']) and torch.equal(frozen['out'], full['out'])
    names = _kernels_of(lambda: _module_run(name, True, input_grad=True, frozen=True))
    assert any('k_stem_gnb_dh' in k for k in names) and any('k_stem_conv0_dgrad' in k for k in names), names
    bad = [k for k in names if any(s in k for s in ('wgrad', 'k_stem_reduce', 'miopen', 'igemm', 'native_group_norm'))]
    assert not bad, bad


@pytest.mark.parametrize('name', ['s64_f128', 's102_f64'])
def test_two_runs_give_the_same_bits(name):
    a = _module_run(name, False)
    b = _module_run(name, False)
    assert len(a) == 18
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_guard_bands_around_workspace_outputs_and_inputs():
    """(1, 3, 51, 51) -> 64 in 16-pixel bands (2401 = 150 x 16 + 1): workspace, output and every gradient between bands of test-owned
    bytes, fills 0xFF and 0x7F; inputs embedded likewise.  tests/guarded.py."""
    from neural_ode_features_amd import stem as S
    from tests import guarded
    name = 's51_f64'
    mod, x, cot = B.reference(name, False)['inputs']

    def build():
        return [x, cot] + [p.detach().clone() for p in S._params_of(mod)]

    def run(tensors):
        stem = _on_gpu(mod)
        stem.input_grad = True
        with torch.no_grad():
            for p, t in zip(S._params_of(stem), tensors[2:]):
                p.data = t
        xg = tensors[0].requires_grad_(True)
        out = stem(xg)
        assert type(out.grad_fn).__name__ == '_BandedStemFnBackward'
        out.backward(tensors[1])
        res = [out.detach(), xg.grad] + [p.grad for p in S._params_of(stem)]
        xg.requires_grad_(False)
        return res

    case = guarded.Case('banded stem ' + name, build, run, calls=['node_stem_banded_fwd', 'node_stem_banded_bwd_dx'],
                        bytes_fn='node_stem_banded_workspace_bytes', pools=[S._BANDED_WS], outputs=[(tuple(cot.shape), torch.float32)])
    with tune_env(NODE_TUNE_STEM_BAND_PX=16):
        plain = guarded.plain_run(case, 'cuda')
        for fill in (0xFF, 0x7F):
            guarded.guarded_run(case, fill, plain, 'cuda')


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_model_takes_the_banded_node_on_64_pixel_images_and_only_there(monkeypatch):
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import stem as S
    monkeypatch.setattr(S.ResidualStem, 'fused_banded', True)
    torch.manual_seed(3)
    net = nof.ODENet(3, n_filters=64, downsample='residual').cuda()
    stem = net.downsample.module
    x64 = torch.randn(2, 3, 64, 64, device='cuda')
    assert type(stem(x64).grad_fn).__name__ == '_BandedStemFnBackward'
    assert type(stem(x64[:, :, :32, :32].contiguous()).grad_fn).__name__ == '_StemFnBackward'
    monkeypatch.setattr(S.ResidualStem, 'fused_banded', False)
    off = stem(x64)
    assert type(off.grad_fn).__name__ not in ('_BandedStemFnBackward', '_StemFnBackward')
    monkeypatch.setattr(S.ResidualStem, 'fused_banded', True)
    on = stem(x64)
    assert float((on - off).abs().max() / off.abs().max()) <= 1e-4       # (the modules run MIOpen / ATen in fp32)
    # the whole net: logits and a backward through node and solve
    logits = net(x64)
    logits.sum().backward()
    assert bool(torch.isfinite(logits).all()) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in stem.parameters())


def test_bim_on_64_pixel_images_matches_the_fp64_loop(monkeypatch):
    """Two L2 iterations of attack.bim on [2, 3, 64, 64] (the image gradient through node_stem_banded_bwd_dx with frozen parameters)
    against attack.bim_reference on the fp64 comparator, to the bound of tests/test_gpu_attack.py's L2 cases, whose net, images and
    comparator these are."""
    from neural_ode_features_amd import stem as S
    from neural_ode_features_amd.attack import bim, bim_reference
    from tests.test_gpu_attack import CIFAR, RefODENet, _images, _net, _normalise
    monkeypatch.setattr(S.ResidualStem, 'fused_banded', True)
    net = _net(0)
    ref = RefODENet(net)
    x = _images(0, n=2, side=64)
    with torch.no_grad():
        labels = ref(_normalise(x.double(), CIFAR)).argmax(1)
    kw = dict(epsilon=.05, stepsize=.02, iterations=2)
    ref.margins = []
    want = bim_reference(ref, x.double(), labels, norm=2, return_early=False, preprocessing=CIFAR, **kw)
    print('fp64 loop: smallest top-2 margin %.2e, found at %s' % (min(ref.margins), want.found_iteration.tolist()))
    assert min(ref.margins) >= 1e-3
    net = net.cuda()
    seen = []
    hook = net.downsample.module.register_forward_hook(lambda m, i, o: seen.append(type(o.grad_fn).__name__))
    got = bim(net, x.cuda(), labels.cuda(), norm=2, return_early=False, preprocessing=CIFAR, **kw)
    hook.remove()
    assert '_BandedStemFnBackward' in seen and '_StemFnBackward' not in seen, seen
    assert net.downsample.module.input_grad is False and all(p.requires_grad for p in net.parameters())
    assert got.adversarial_class.cpu().tolist() == want.adversarial_class.tolist()
    assert got.found_iteration.cpu().tolist() == want.found_iteration.tolist()
    derr = float((got.distance.cpu().double() - want.distance).abs().max())
    xerr = float((got.adversarial.cpu().double() - want.adversarial).abs().max())
    print('bim on 64 x 64: image error %.2e, distance error %.2e' % (xerr, derr))
    assert derr <= 1e-5 and xerr <= 1e-5, (derr, xerr)

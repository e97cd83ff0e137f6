"""The GroupNorm residual stem and the residual trunk (csrc/kernels_stem.hip, csrc/stem_api.hip, csrc/trunk_api.hip) on the
geometries of tests/stem_geometry_cases.py: rectangular and odd images, every channel block of the GroupNorm passes (8 ... 128),
16 and 32 channels per group, the 2400-pixel ceiling and the 5 x 5 floor, the F(4x4,3x3) last layer behind a rectangular image.
What each case reaches is asserted against the library's probes there and in tests/test_stem_geometry_host.py.

Every case runs through the C ABI (node_stem_fwd, node_stem_bwd, node_stem_bwd_dx / node_trunk_fwd, node_trunk_bwd) with a workspace
of its own that starts as 0xFF bytes, once with NODE_TUNE_STEM_GN=0 (k_stem_gn_fwd / k_stem_gn_bwd) and once by default
(k_stem_gn_*_fl); the two CPU runs and the GPU runs are computed once per case and shared by the tests.

Against the truth: the output, every parameter gradient and the input gradient against the same modules in float64 on the CPU, per
tensor in max norm relative to max |fp64|.  The bound is 8 x max(the fp32 CPU run's distance from fp64 for that tensor, 2^-24) -- the
rule of tests/test_gpu_step_control.py and tests/test_gpu_stem_gn_paths.py, computed here and never taken from the code under test;
the floor keeps a tensor the CPU happens to get exactly right from demanding zero.  Where the last convolution takes the
F(4x4,3x3) pipeline (fp16-pair or bf16 component GEMMs), its weight gradient and everything upstream of it in the backward -- that is
every gradient but b2_ds_w's -- are held to the bounds tests/test_gpu_stem.py sets for that path (5e-5) and the output to 2e-5.

Old path against new: outputs, gradients and the whole workspace behind the forward and behind each backward, byte for byte."""
import copy

import pytest
import torch

from tests import stem_geometry_cases as G

gpu = pytest.mark.gpu
_cache = {}
W4_OUT_BOUND, W4_GRAD_BOUND = 2e-5, 5e-5          # tests/test_gpu_stem.py, the F(4x4,3x3) last layer
B2_DS_W = 'grad15'                                # the second shortcut's filter: its gradient reads dL/d out and a2 only


def _gpu_dims(kind, row):
    a, h, w, c, n = row['dims']
    return (n, a, h, w, c)


def _results(case, monkeypatch):
    """fp64, fp32 CPU, GPU old path, GPU new path: computed once per case, shared by the tests, never changed."""
    if case not in _cache:
        from tests.helpers import stem_family_gpu_run
        kind, row, env = G.row_of(case)
        refs = G.references(case)
        _, mod, order, x, cot = refs['inputs']
        for k in ('NODE_TUNE_STEM_W4', 'NODE_TUNE_STEM_GN'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        p = G.assert_claim(case)              # in this process, under this environment
        r = {'ref': refs['ref'], 'cpu32': refs['cpu32'], 'plan': p}
        monkeypatch.setenv('NODE_TUNE_STEM_GN', '0')
        r['old'] = stem_family_gpu_run(kind, _gpu_dims(kind, row), mod, order, x, cot, with_dx=kind == 'stem')
        monkeypatch.delenv('NODE_TUNE_STEM_GN')
        r['new'] = stem_family_gpu_run(kind, _gpu_dims(kind, row), mod, order, x, cot, with_dx=kind == 'stem')
        _cache[case] = r
    return _cache[case]


def _words(t):
    return t.contiguous().view(torch.uint8)


@gpu
@pytest.mark.parametrize('case', G.CASES)
def test_new_path_writes_the_old_path_bits(case, monkeypatch):
    r = _results(case, monkeypatch)
    old, new = r['old'], r['new']
    assert set(old) == set(new)
    differ = []
    for key in sorted(old):
        if not key.startswith('ws'):
            for path in (old, new):
                assert not torch.isnan(path[key]).any(), (case, key, 'left unwritten')
        if not torch.equal(_words(old[key]), _words(new[key])):
            diff = (_words(old[key]) != _words(new[key])).nonzero().flatten()
            print('%s %s: %d bytes differ, first at byte %d, last at %d of %d'
                  % (case, key, diff.numel(), int(diff[0]), int(diff[-1]), _words(old[key]).numel()))
            differ.append(key)
    assert not differ, (case, differ)
    start = torch.full_like(old['ws_fwd'], 0xFF)
    frac = lambda a, b: int(torch.count_nonzero(a != b)) / a.numel()
    written, rewritten = frac(old['ws_fwd'], start), frac(old['ws_bwd'], old['ws_fwd'])
    print('%s: the forward wrote %.0f %% of the workspace bytes, the backward changed %.0f %%' % (case, 100 * written, 100 * rewritten))
    assert written > 0.1 and rewritten > 0.01


@gpu
@pytest.mark.parametrize('case', [c for c in G.CASES if G.row_of(c)[0] == 'stem'])
def test_bwd_dx_returns_the_parameter_gradients_of_bwd(case, monkeypatch):
    """node_stem_bwd_dx behind node_stem_bwd on the same workspace: the sixteen gradients bit for bit (include/node_hip.h)."""
    r = _results(case, monkeypatch)
    for path in ('old', 'new'):
        for i in range(16):
            assert torch.equal(_words(r[path]['grad%02d' % i]), _words(r[path]['dxgrad%02d' % i])), (case, path, i)


def _bound(case, key, r):
    """(bound, what it is) of a tensor of a case"""
    ref, cpu32 = r['ref'], r['cpu32']
    scale = float(ref[key].abs().max())
    own = 8 * max(float((cpu32[key] - ref[key]).abs().max()) / scale, 2.0 ** -24)
    if r['plan']['w4'] and key != B2_DS_W:
        return (W4_OUT_BOUND if key == 'out' else W4_GRAD_BOUND), 'F(4x4,3x3) path'
    return own, '8 x fp32 CPU'


@gpu
@pytest.mark.parametrize('case', G.CASES)
def test_both_paths_match_fp64_within_eight_times_the_fp32_cpu_distance(case, monkeypatch):
    r = _results(case, monkeypatch)
    ref = r['ref']
    keys = sorted(k for k in ref if k != 'u')
    assert len(keys) == (18 if G.row_of(case)[0] == 'stem' else 6 * G.row_of(case)[1]['dims'][3] + 2)
    worst, lines = {}, []
    for key in keys:
        scale = float(ref[key].abs().max())
        assert scale > 0, (case, key)
        bound, what = _bound(case, key, r)
        for path in ('new', 'old'):
            assert r[path][key].shape == ref[key].shape
            err = float((r[path][key].double() - ref[key]).abs().max()) / scale
            lines.append('%s %-7s %s: error %.3e, bound %.3e (%s)' % (case, key, path, err, bound, what))
            worst[(key, path)] = (err, bound)
    print('\n'.join(lines))                 # (profiles/stem_geometry_parity.txt is this output)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


@gpu
@pytest.mark.parametrize('case', ['r51x47_f256', 's5_f256', 'r31x34_f128_n8'])
def test_the_module_takes_the_fused_node_and_returns_the_abi_bits(case, monkeypatch):
    r = _results(case, monkeypatch)
    for k in ('NODE_TUNE_STEM_W4', 'NODE_TUNE_STEM_GN'):
        monkeypatch.delenv(k, raising=False)
    _, mod, order, x, cot = G.references(case)['inputs']
    stem = copy.deepcopy(mod).cuda()
    out = stem(x.cuda())
    assert type(out.grad_fn).__name__ == '_StemFnBackward'          # the fused node, not the module sequence
    assert torch.equal(_words(out.detach().cpu()), _words(r['new']['out']))
    out.backward(cot.cuda())
    for i, p in enumerate(order(stem)):
        assert torch.equal(_words(p.grad.cpu()), _words(r['new']['grad%02d' % i])), (case, i)


@gpu
def test_one_pixel_past_the_ceiling_runs_the_module_sequence():
    """3 x 51 x 51: 49 x 49 = 2401 pixels behind the first layer.  The library refuses it (tests/test_stem_geometry_host.py), the Python
    gate sends it to the module sequence, and that still matches fp64 to the bound of
    test_stem_filter_counts_the_kernels_refuse_run_the_module_sequence (tests/test_gpu_stem.py)."""
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import stem as S
    torch.manual_seed(3)
    mod = nof.ODENet(3, out=10, n_filters=64, downsample='residual', adjoint=True).downsample.module
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(1, 3, 51, 51, generator=gen)
    stem = copy.deepcopy(mod).cuda()
    assert not S.fusable(stem, x.cuda()) and S.fusable(stem, x[:, :, :50, :].cuda())
    assert S.fusable(stem, torch.randn(2, 3, 5, 5).cuda()) and not S.fusable(stem, torch.randn(2, 3, 5, 4).cuda())
    out = stem(x.cuda())
    assert type(out.grad_fn).__name__ != '_StemFnBackward'
    ref = copy.deepcopy(mod).double()
    out_ref = ref(x.double())
    cot = torch.randn(out_ref.shape, generator=gen)
    out.backward(cot.cuda())
    out_ref.backward(cot.double())
    assert float((out.detach().cpu().double() - out_ref.detach()).abs().max() / out_ref.detach().abs().max()) <= 1e-4
    for (name, p), (_, q) in zip(stem.named_parameters(), ref.named_parameters()):
        assert float((p.grad.cpu().double() - q.grad).norm() / q.grad.norm()) <= 1e-3, name

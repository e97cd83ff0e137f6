"""The GroupNorm + ReLU passes of the stem kernels (csrc/kernels_stem.hip) on their two launch paths: the default
(`k_stem_gn_fwd_fl` / `k_stem_gn_bwd_fl`: batched fills, read-ahead sums, store loops on registers) against
`NODE_TUNE_STEM_GN=0` (`k_stem_gn_fwd` / `k_stem_gn_bwd`, the kernels as they were), through the entry points the stem and trunk
tests use (node_stem_fwd / node_stem_bwd, node_trunk_fwd / node_trunk_bwd).  The library has no entry for a GroupNorm pass
alone, so a case is a whole node at batch 2 and what is compared is everything the node writes: its outputs, every gradient and
the WHOLE workspace after the forward and after the backward, byte for byte -- the workspace is where the passes' triples
(three planes), `stats`, `gpart` and fp32 `dh` live.  Workspace and outputs start as 0xFF bytes (NaN in fp32 and bf16).

Cases (HW, C, channels per group), at N = 2:
  stem 3 x 32 x 32, filters 256:  (30.30, 64, 2)  (15.15, 64, 2) twice  (8.8, 256, 8)
  stem 1 x 28 x 28, filters 64:   (26.26, 64, 2)  (13.13, 64, 2) twice  (7.7, 64, 2)
  trunk 256 x 8 x 8, two blocks:  (8.8, 256, 8) with SKIP = true (every block's first norm) and without (its second)
and at N = 5, stem 3 x 32 x 32, filters 64: the 30.30 launches are 20 workgroups, a grid above 8 that is no multiple
of 8 -- where the new kernels' block id (gn_block_id) is neither the identity nor the even deal.
30.30 x 16 channels is 3600 fill requests = 1 batch of 8 x 256 and a partial one; 7.7 x 64 is 784 = a partial batch alone, 49
pixels per thread class of 4; 8.8 x 128 is exactly one batch and nothing behind it.  Backward output forms: the stem writes triples only (three
launches) and fp32 only (the first norm); the trunk's SKIP launches write fp32 only (block 0) and both (block 1), its
other launches triples only.

Against the truth: outputs and gradients of BOTH paths against the same modules in float64 on the CPU
(`torch.nn.functional.group_norm` + ReLU + the convolutions, and autograd), per tensor in max norm relative to max |fp64|;
the bound is 8 x the distance of the fp32 CPU run of the same modules from fp64, computed here for each tensor (the rule of
tests/test_gpu_step_control.py), so it never comes from the code under test."""
import copy
import ctypes as C

import pytest
import torch

gpu = pytest.mark.gpu

CASES = {'stem32_f256': ('stem', 3, 32, 256, 2), 'stem28_f64': ('stem', 1, 28, 64, 2), 'trunk8_c256': ('trunk', 256, 8, 2, 2),
         'stem32_f64_n5': ('stem', 3, 32, 64, 5)}
_cache = {}


def _perturb_norms(mod, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if 'norm' in name:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))


def _modules(case):
    """(fp32 module, its ordered parameter list function, input, cotangent) of a case, on the CPU"""
    import neural_ode_features_amd as nof
    kind, a, b, c, N = CASES[case]
    torch.manual_seed(len(case) + a + b + c)
    gen = torch.Generator().manual_seed(17 + a + b + c)
    if kind == 'stem':
        from neural_ode_features_amd import stem as S
        mod = nof.ODENet(a, out=10, n_filters=c, downsample='residual', adjoint=True).downsample.module
        x = torch.randn(N, a, b, b, generator=gen)
        order = S._params_of
    else:
        from neural_ode_features_amd import resnet as R
        mod = nof.ResidualTrunk(a, c)
        x = torch.randn(N, a, b, b, generator=gen)
        order = R._params_of
    _perturb_norms(mod, 5 + a + b + c)
    with torch.no_grad():
        shape = mod(x).shape
    cot = torch.randn(shape, generator=gen)
    return kind, mod, order, x, cot


def _cpu_run(mod, order, x, cot, dtype, want_dx):
    m = copy.deepcopy(mod).to(dtype)
    xin = x.to(dtype).requires_grad_(want_dx)
    out = m(xin)
    out.backward(cot.to(dtype))
    res = {'out': out.detach().double()}
    for i, p in enumerate(order(m)):
        res['grad%02d' % i] = p.grad.double()
    if want_dx:
        res['dx'] = xin.grad.double()
    return res


def _gpu_run(case, kind, mod, order, x, cot):
    """One forward and one backward through the C ABI with a workspace of our own: outputs, gradients and the workspace's bytes
    (tests/helpers.py: stem_family_gpu_run, shared with tests/test_gpu_stem_geometry.py)."""
    from tests.helpers import stem_family_gpu_run
    _, a, b, c, N = CASES[case]
    return stem_family_gpu_run(kind, (N, a, b, b, c), mod, order, x, cot)


def _results(case, monkeypatch):
    """fp64, fp32 CPU, GPU old path, GPU new path: computed once per case, shared by the tests, never changed."""
    if case not in _cache:
        kind, mod, order, x, cot = _modules(case)
        want_dx = kind == 'trunk'
        r = {'ref': _cpu_run(mod, order, x, cot, torch.float64, want_dx), 'cpu32': _cpu_run(mod, order, x, cot, torch.float32, want_dx)}
        monkeypatch.setenv('NODE_TUNE_STEM_GN', '0')
        r['old'] = _gpu_run(case, kind, mod, order, x, cot)
        monkeypatch.delenv('NODE_TUNE_STEM_GN')
        r['new'] = _gpu_run(case, kind, mod, order, x, cot)
        _cache[case] = r
    return _cache[case]


def _words(t):
    return t.contiguous().view(torch.uint8)


@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_new_path_writes_the_old_path_bits(case, monkeypatch):
    r = _results(case, monkeypatch)
    old, new = r['old'], r['new']
    assert set(old) == set(new)
    differ = []
    for key in sorted(old):
        if not key.startswith('ws'):
            assert not torch.isnan(new[key]).any(), (case, key, 'left unwritten')
        if not torch.equal(_words(old[key]), _words(new[key])):
            diff = (_words(old[key]) != _words(new[key])).nonzero().flatten()
            print('%s %s: %d bytes differ, first at byte %d, last at %d of %d'
                  % (case, key, diff.numel(), int(diff[0]), int(diff[-1]), _words(old[key]).numel()))
            differ.append(key)
    assert not differ, (case, differ)
    # the workspace did take the passes' results: a large part of it changed in each direction
    start = torch.full_like(old['ws_fwd'], 0xFF)
    written, rewritten = float((old['ws_fwd'] != start).float().mean()), float((old['ws_bwd'] != old['ws_fwd']).float().mean())
    print('%s: the forward wrote %.0f %% of the workspace bytes, the backward changed %.0f %%' % (case, 100 * written, 100 * rewritten))
    assert written > 0.1 and rewritten > 0.01


@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_both_paths_match_fp64_within_eight_times_the_fp32_cpu_distance(case, monkeypatch):
    r = _results(case, monkeypatch)
    ref, cpu32 = r['ref'], r['cpu32']
    worst = {}
    for key in sorted(ref):
        scale = float(ref[key].abs().max())
        bound = 8 * float((cpu32[key] - ref[key]).abs().max()) / scale
        for path in ('new', 'old'):
            err = float((r[path][key].double() - ref[key]).abs().max()) / scale
            print('%s %-7s %s: error %.3e, bound %.3e (8 x fp32 CPU)' % (case, key, path, err, bound))
            worst[(key, path)] = (err, bound)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


def _gn_cb(hw, c, cpg):
    """stem_gn_cb (csrc/kernels_stem.hip), restated; the host test below holds the restatement to the library's own answer
    (node_stem_describe) and checks the refusal (workspace size 0) and the acceptance (> 0) of node_stem_workspace_bytes."""
    budget = 150 * 1024
    cb = 8
    while cb < cpg:
        cb *= 2
    if cb > c or cb > 128 or hw * cb * 2 * 4 > budget:
        return 0
    while cb * 2 <= c and cb * 2 <= 128 and hw * cb * 4 * 4 <= budget:
        cb *= 2
    return cb if c % cb == 0 and cb % cpg == 0 else 0


def test_channel_blocks_keep_whole_groups_and_refused_shapes_stay_refused():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    St = _lib.NodeStemShape
    for filters in (192, 384):
        assert lib.node_stem_workspace_bytes(C.byref(St(2, 3, 32, 32, filters, 1e-5))) == 0
        assert _gn_cb(8 * 8, filters, filters // 32) == 0
    for filters in (64, 256):
        assert lib.node_stem_workspace_bytes(C.byref(St(2, 3, 32, 32, filters, 1e-5))) > 0
        for hw, c in ((30 * 30, 64), (15 * 15, 64), (8 * 8, filters)):
            cpg = c // 32
            cb = _gn_cb(hw, c, cpg)
            assert cb >= 8 and c % cb == 0 and cb % cpg == 0 and 256 % cb == 0
            assert (2 * hw * cb + 1024) * 4 <= 160 * 1024           # the backward's two tiles and its scratch fit a CU's LDS
        assert [g['cb'] for g in _lib.stem_plan(2, 3, 32, 32, filters)['gn']] == [_gn_cb(30 * 30, 64, 2), _gn_cb(15 * 15, 64, 2),
                                                                                 _gn_cb(15 * 15, 64, 2), _gn_cb(8 * 8, filters, filters // 32)]

"""The cases of the block-wise parameter-gradient tests: which shape, under which NODE_TUNE_* switches, is claimed to run which
kernel instance -- and the code that checks a case (shared by tests/test_gpu_param_grads.py, its child processes and
tests/test_gpu_forced_tiles.py).

Every row names the two instances `node_describe_dims` must report for it (`_lib.WGRAD_KERNELS` / `_lib.CONV_KERNELS`, the
NODE_WGRAD_* / NODE_CONV_* enums of include/node_hip.h) and the K-split count.  tests/test_kernel_selection_host.py asserts the
whole table without a GPU, each switch set in a process of its own (the switches are read once per process); every GPU case
asserts its own row again before it launches anything.  `coverage()` is the claim that the rows together reach every value of
both enums.

Run as a child:  python -c "from tests.param_grad_cases import main; main()" GROUP [--select-only]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WGRAD_KERNELS = ('W2_8', 'W2_4', 'W_8_8', 'W_16_2', 'W_4_4', 'T_8_8', 'T_16_4', 'T_7_7', 'T_4_4', 'P')
CONV_KERNELS = ('DIRECT_64', 'DIRECT_128', 'DIRECT_256', 'W1_64', 'W1_128', 'W1_256', 'W2_128')

# Bounds (the project's existing ones; nothing here is measured from a kernel): rel_err of f, vjp_y and the flat parameter
# gradient, |vjp_t - ref| relative to |ref|, and the per-block bound relative to each block's own scale (tests/helpers.py).
BOUNDS_FP32 = dict(f=2e-5, vy=5e-5, vp=5e-5, vt=1e-4, block=5e-5)
BOUNDS_W4 = dict(f=3e-5, vy=1e-4, vp=1e-4, vt=1e-4, block=1e-4)       # the F(4x4,3x3) pipeline (tests/test_gpu_w4.py)


def row(shape, wgrad, conv, nsplit, why, **more):
    return dict(shape=tuple(shape), wgrad=wgrad, conv=conv, nsplit=nsplit, why=why, **more)


# ---- no switch: what a shape selects by itself ------------------------------------------------------------------------------
DEFAULT = [
    # 2-D Winograd-domain weight gradient, units of 8 tiles
    row((1, 64, 8, 8), 'W2_8', 'W1_64', 2, 'nsplit clamped to the 2 units of one sample'),
    row((9, 128, 8, 8), 'W2_8', 'W1_64', 18, 'four channel-tile pairs, 18 units in 18 splits; 4 channels / group'),
    row((33, 64, 8, 8), 'W2_8', 'W1_64', 32, 'nsplit capped at 32: 66 units in ragged shares of 3 and 2'),
    row((3, 160, 8, 8), 'W2_8', 'W1_64', 6, 'ntc = 3 with a ragged 32-channel last tile; 5 channels / group'),
    row((2, 96, 8, 8), 'W2_8', 'W1_64', 4, 'ragged 64-channel tile; 3 channels / group (N tile of 63 columns)'),
    row((3, 32, 4, 8), 'W2_8', 'W1_64', 3, 'one unit per sample: 4x8'),
    row((2, 32, 8, 4), 'W2_8', 'W1_64', 2, 'units of 8 tiles = four tile rows of width 2'),
    row((2, 32, 16, 16), 'W2_8', 'W2_128', 16, '16x16: eight units per sample, conv in two bands per sample'),
    row((3, 256, 8, 8), 'W2_8', 'W1_64', 6, '8 channels / group'),
    # ... units of 4 tiles
    row((3, 64, 4, 4), 'W2_4', 'W1_64', 3, 'one unit of 4 tiles per sample; three samples in a 64-row conv tile'),
    row((2, 32, 2, 8), 'W2_4', 'W1_64', 2, 'a single tile row'),
    row((2, 32, 12, 4), 'W2_4', 'W1_64', 6, 'three units per sample, 48 pixels'),
    row((2, 768, 4, 4), 'W2_4', 'W1_64', 1, 'nsplit == 1 (144 channel-tile pairs)'),
    row((2, 512, 4, 4), 'W2_4', 'W1_64', 2, '16 channels / group'),
    row((1, 1024, 4, 4), 'W2_4', 'W1_64', 1, '32 channels / group'),
    # k_wgrad_t<7,7>
    row((5, 64, 7, 7), 'T_7_7', 'DIRECT_64', 5, 'the MNIST state: odd width, direct conv at 64-row tiles'),
    row((2, 8, 7, 7), 'T_7_7', 'DIRECT_64', 2, 'C < one K chunk, 1 channel / group'),
    # k_wgrad_p
    row((3, 16, 5, 6), 'P', 'W1_64', 3, 'non-square, odd height'),
    row((2, 32, 6, 6), 'P', 'W1_64', 2, 'odd number of column pairs'),
    row((2, 32, 12, 12), 'P', 'W1_256', 6, '144 pixels in a 256-row tile; ragged last band'),
    row((2, 16, 10, 14), 'P', 'W1_256', 6, 'non-square, 7 column pairs'),
    row((2, 32, 7, 8), 'P', 'W1_64', 2, 'odd height on an even width'),
    row((7, 16, 2, 2), 'P', 'W1_64', 7, 'seven samples in one conv tile'),
    row((2, 64, 32, 32), 'P', 'W2_128', 32, '32x32: conv in eight bands per sample, one-row wgrad bands'),
    row((3, 128, 16, 32), 'P', 'W2_128', 32, '16x32: four bands per sample, two N tiles'),
    row((3, 32, 6, 16), 'W2_8', 'W1_128', 9, '96 pixels: the 1-D Winograd conv at 128-row tiles'),
    row((2, 32, 9, 9), 'P', 'DIRECT_128', 4, '81 pixels, odd width: the direct conv at 128-row tiles; ragged second wgrad band'),
    row((2, 16, 11, 13), 'P', 'DIRECT_256', 6, '143 pixels, odd width: the direct conv at 256-row tiles'),
    # 2-D Winograd conv at 128-row tiles without forcing
    row((3, 32, 8, 16), 'W2_8', 'W2_128', 12, 'one sample per 128-row tile'),
]

# ---- the F(4x4,3x3) pipeline (NODE_TUNE_WINO4=2, read per call): its own GEMMs and passes in place of the fp32 conv, and for
# C % 128 == 0 its own weight gradient; each case runs on bf16 triples (NODE_TUNE_W4_F16=0) and with the fp16 pairs allowed (=1)
W4 = [
    row((8, 64, 8, 8), 'W2_8', 'W1_64', 16, 'C = 64: the F(2x2,3x3)-domain weight gradient behind the pipeline', w4=1),
    row((3, 128, 8, 8), 'W2_8', 'W1_64', 6, 'batch padded to 8; F(4x4,3x3)-domain weight gradient', w4=1),
    row((12, 256, 8, 8), 'W2_8', 'W1_64', 8, 'batch padded to 16', w4=1),
    row((1, 128, 16, 16), 'W2_8', 'W2_128', 8, 'four quadrants of one image', w4=1),
    row((2, 512, 16, 16), 'W2_8', 'W2_128', 2, 'the LDS-tiled weight gradient (C >= 512); 16 channels / group', w4=1),
]

# ---- the kernels behind the once-per-process switches: (group, switches, rows) -------------------------------------------------
_TILES = [(5, 64, 8, 8), (16, 32, 4, 4), (3, 32, 4, 8), (7, 96, 8, 8), (33, 64, 8, 8)]      # test_gpu_forced_tiles.py's list
_NS_TILES = [10, 16, 3, 14, 32]


def _conv_rows(conv):
    wg = ['W2_8', 'W2_4', 'W2_8', 'W2_8', 'W2_8']
    return ([row(s, w, conv, n, 'forced conv family / tile') for s, w, n in zip(_TILES, wg, _NS_TILES)] +
            [row((2, 32, 5, 8), 'P', conv, 2, 'odd height on an even width')])


CHILDREN = [
    ('wgrad_w', dict(NODE_TUNE_WGRAD_WINO='1'), [
        row((5, 64, 8, 8), 'W_8_8', 'W1_64', 5, 'k_wgrad_w<8,8>'),
        row((2, 32, 16, 8), 'W_8_8', 'W2_128', 4, 'k_wgrad_w<8,8>, two bands per sample'),
        row((2, 32, 16, 16), 'W_16_2', 'W2_128', 16, 'k_wgrad_w<16,2>'),
        row((3, 32, 6, 16), 'W_16_2', 'W1_128', 9, 'k_wgrad_w<16,2>, three bands per sample'),
        row((3, 64, 4, 4), 'W_4_4', 'W1_64', 3, 'k_wgrad_w<4,4>'),
        row((2, 96, 8, 4), 'W_4_4', 'W1_64', 4, 'k_wgrad_w<4,4>, two bands per sample, ragged channel tile')]),
    ('wgrad_t', dict(NODE_TUNE_WGRAD_WINO='0'), [
        row((5, 64, 8, 8), 'T_8_8', 'W1_64', 5, 'k_wgrad_t<8,8>'),
        row((2, 32, 16, 8), 'T_8_8', 'W2_128', 4, 'k_wgrad_t<8,8>, two bands per sample'),
        row((2, 32, 16, 16), 'T_16_4', 'W2_128', 8, 'k_wgrad_t<16,4>'),
        row((2, 32, 4, 16), 'T_16_4', 'W1_64', 2, 'k_wgrad_t<16,4>, one band per sample'),
        row((3, 64, 4, 4), 'T_4_4', 'W1_64', 3, 'k_wgrad_t<4,4>'),
        row((16, 32, 4, 4), 'T_4_4', 'W1_64', 16, 'k_wgrad_t<4,4>, 16 units')]),
    ('wgrad_p', dict(NODE_TUNE_WGRAD_WINO='0', NODE_TUNE_WGRAD_VARIANT='0'), [
        row((5, 64, 8, 8), 'P', 'W1_64', 5, 'k_wgrad_p at 8x8'),
        row((2, 32, 16, 16), 'P', 'W2_128', 8, 'k_wgrad_p at 16x16'),
        row((3, 64, 4, 4), 'P', 'W1_64', 3, 'k_wgrad_p at 4x4'),
        row((5, 64, 7, 7), 'P', 'DIRECT_64', 5, 'k_wgrad_p at 7x7')]),
    ('conv_direct_64', dict(NODE_TUNE_CONV_WINO='0', NODE_TUNE_CONV_BM='64'), _conv_rows('DIRECT_64')),
    ('conv_direct_128', dict(NODE_TUNE_CONV_WINO='0', NODE_TUNE_CONV_BM='128'), _conv_rows('DIRECT_128')),
    ('conv_w1_64', dict(NODE_TUNE_CONV_WINO='1', NODE_TUNE_CONV_BM='64'), _conv_rows('W1_64')),
    ('conv_w1_128', dict(NODE_TUNE_CONV_WINO='1', NODE_TUNE_CONV_BM='128'), _conv_rows('W1_128')),
]
# tests/test_gpu_forced_tiles.py::test_2d_winograd_conv_on_small_batches (kink-free parameters, as that test always used)
FORCED_W2 = ('conv_w2_128', dict(NODE_TUNE_CONV_WINO='2', NODE_TUNE_CONV_BM='128'),
             [row(s, w, 'W2_128', n, 'forced 2-D Winograd conv at 128-row tiles', kink_free=True)
              for s, w, n in zip(_TILES, ['W2_8', 'W2_4', 'W2_8', 'W2_8', 'W2_8'], _NS_TILES)])

GROUPS = dict([('default', (dict(), DEFAULT)), ('w4', (dict(), W4))] + [(g, (e, r)) for g, e, r in CHILDREN + [FORCED_W2]])

# Every switch a row's selection depends on: a group's process must have exactly its own set
SWITCHES = ('NODE_TUNE_WGRAD_WINO', 'NODE_TUNE_WGRAD_VARIANT', 'NODE_TUNE_CONV_WINO', 'NODE_TUNE_CONV_BM', 'NODE_TUNE_SMALL',
            'NODE_TUNE_TINY')

# Values of the two enums that no row reaches, each with its reason.  (None: every instance has a small shape, by default or
# behind a switch.  What has none is a ROUTE, not an instance: a tensor of >= 2^32 bytes leaves the 2-D Winograd weight gradient
# for k_wgrad_w<8,8> / <16,2> / <4,4>, and the 2-D Winograd conv for the 1-D one -- the same instances the `wgrad_w` and `conv_w1_*`
# groups reach by switch -- and such a tensor cannot be small.)
NOT_REACHED = {}


def coverage():
    """(wgrad instances, conv instances) the rows claim, each mapped to the groups that reach it."""
    wg, cv = {}, {}
    for g, (_, rows) in GROUPS.items():
        if g == 'w4':
            continue          # (the pipeline replaces the fp32 conv; its rows claim the instances only as the geometry's selection)
        for r in rows:
            wg.setdefault(r['wgrad'], set()).add(g)
            cv.setdefault(r['conv'], set()).add(g)
    return wg, cv


def check_coverage():
    wg, cv = coverage()
    missing = [k for k in WGRAD_KERNELS if k not in wg and k not in NOT_REACHED] + [k for k in CONV_KERNELS if k not in cv and k not in NOT_REACHED]
    assert not missing, 'kernel instances no case reaches and NOT_REACHED does not explain: %s' % missing
    assert not (set(wg) | set(cv)) - set(WGRAD_KERNELS) - set(CONV_KERNELS)
    return wg, cv


check_coverage()          # at import: a table that loses an instance fails every test that uses it


def kink_free(r):
    """Ordinary parameters (live ReLU masks) below 10^5 state elements, the kink-free set from there on -- as, and for the reason,
    tests/test_gpu_parity.py states."""
    n, c, h, w = r['shape']
    return bool(r.get('kink_free')) or n * c * h * w >= 100000


def _lib_module():
    """The ctypes binding by file, without importing the package (and torch): the selection needs neither."""
    import importlib.util
    name = 'neural_ode_features_amd._lib'
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location('_node_lib_standalone', os.path.join(ROOT, 'neural-ode-features_amd', '_lib.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assert_selection(r, lib=None):
    """The row's claim against node_describe_dims in THIS process."""
    lib = lib or _lib_module()
    assert tuple(lib.WGRAD_KERNELS) == WGRAD_KERNELS and tuple(lib.CONV_KERNELS) == CONV_KERNELS
    if r.get('w4'):
        old = os.environ.get('NODE_TUNE_WINO4')
        os.environ['NODE_TUNE_WINO4'] = '2'
    try:
        d = lib.describe_dims(*r['shape'])
    finally:
        if r.get('w4'):
            if old is None:
                del os.environ['NODE_TUNE_WINO4']
            else:
                os.environ['NODE_TUNE_WINO4'] = old
    got = (d['wgrad_kernel'], d['conv_kernel'], d['nsplit'])
    assert got == (r['wgrad'], r['conv'], r['nsplit']), (r['shape'], 'claimed', (r['wgrad'], r['conv'], r['nsplit']), 'selected', got, d)
    assert not r.get('w4') or d['wino4'] == 2, (r['shape'], d)
    return d


def assert_group_environment(group):
    env = GROUPS[group][0]
    for k in SWITCHES:
        assert os.environ.get(k) == env.get(k), 'group %s needs %s=%s, the process has %s' % (group, k, env.get(k), os.environ.get(k))


_REFS = {}


def reference(r, t):
    """(y, cot, the fp64 reference) of a row, computed once per process and left unchanged."""
    import torch
    from tests.helpers import make_func, odefunc_vjp_ref64
    key = (r['shape'], kink_free(r), t)
    if key not in _REFS:
        N, C, H, W = r['shape']
        _, twin = make_func(C, seed=C + H, kink_free=kink_free(r))
        gen = torch.Generator().manual_seed(2)
        y = torch.randn(N, C, H, W, generator=gen)
        cot = torch.randn(N, C, H, W, generator=gen)
        _REFS[key] = (y, cot, odefunc_vjp_ref64(t, y, dict(twin.named_parameters()), cot))
    return _REFS[key]


def run_case(r, group, t=-0.61, env=None, tag='', keep=None):
    """One VJP of the dynamics on the GPU against the fp64 reference: the row's selection first, then f, vjp_y, the flat parameter
    gradient and vjp_t at the project's bounds, then every block at its own scale.  Returns the list of misses (empty: passed);
    `keep` (a dict) receives the GPU's flat parameter gradient."""
    import torch
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import _lib
    from tests.helpers import block_table, emit_table, make_func, rel_err, tune_env, vjp_block_errors
    d = assert_selection(r, _lib)
    bounds = BOUNDS_W4 if r.get('w4') else BOUNDS_FP32
    N, C, H, W = r['shape']
    y, cot, ref = reference(r, t)
    f, _ = make_func(C, seed=C + H, device='cuda', kink_free=kink_free(r))
    with tune_env(**(env or {})):
        fo, vy, vt, vp = nof.odefunc_vjp(f, t, y.cuda(), cot.cuda())
        torch.cuda.synchronize()
    if keep is not None:
        keep['vp'] = vp.detach().cpu()
    errs = dict(f=rel_err(fo, ref['f']), vy=rel_err(vy, ref['vy']), vp=rel_err(vp, ref['vp']),
                vt=abs(float(vt) - ref['vt']) / (abs(ref['vt']) + 1e-6))
    blocks = vjp_block_errors(vp, vt, ref)
    title = '%s %s%s  wgrad %s conv %s nsplit %d%s  %s parameters\n  f %.2e  vjp_y %.2e  flat vjp_params %.2e  vjp_t/|vjp_t| %.2e' % (
        group, r['shape'], tag, d['wgrad_kernel'], d['conv_kernel'], d['nsplit'], '  F(4x4,3x3)' if r.get('w4') else '',
        'kink-free' if kink_free(r) else 'ordinary', errs['f'], errs['vy'], errs['vp'], errs['vt'])
    emit_table(block_table(title, blocks, ref, bounds['block']))
    misses = ['%s %.3e > %.1e' % (k, errs[k], bounds[k]) for k in ('f', 'vy', 'vp', 'vt') if not errs[k] < bounds[k]]
    misses += ['block %s %.3e > %.1e' % (k, e, bounds['block']) for k, e in blocks.items() if not e <= bounds['block']]
    return misses


def main(argv=None):
    """Child process of one switch group: asserts the group's environment and every row's selection; without --select-only runs
    every row on the GPU.  Exit status = number of rows that missed."""
    argv = sys.argv[1:] if argv is None else argv
    group = argv[0]
    assert_group_environment(group)
    rows = GROUPS[group][1]
    if '--select-only' not in argv:
        # PyTorch's HIP runtime first, then the package's binding of the library: the library must find the runtime PyTorch brought
        import torch                                  # noqa: F401
        import neural_ode_features_amd                # noqa: F401
        from neural_ode_features_amd import _lib      # noqa: F401  (what _lib_module() returns from here on)
    for r in rows:
        assert_selection(r)
    if '--select-only' in argv:
        print('selection of group %s: %d rows as claimed' % (group, len(rows)))
        return 0
    bad = 0
    for r in rows:
        misses = run_case(r, group, t=0.41 if group == FORCED_W2[0] else -0.61)
        if misses:
            print('MISS', r['shape'], misses, flush=True)
            bad += 1
    return bad


def child_command(group, select_only=False):
    code = 'import sys; sys.path.insert(0, %r); from tests.param_grad_cases import main; sys.exit(main())' % ROOT
    return [sys.executable, '-c', code, group] + (['--select-only'] if select_only else [])


def child_env(group):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(GROUPS[group][0])
    return env

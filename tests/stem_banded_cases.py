"""The shapes at which tests/test_gpu_stem_banded.py runs the banded residual stem (node_stem_banded_*), and the seed each of them uses
with ordinary parameters -- one table for the host test (tests/test_stem_banded_host.py: the plans, the seed rule) and the GPU test.

Parameters are the stem's own initialisation under `torch.manual_seed(seed)` with the norm weights and biases perturbed by 0.2 randn
(what `_stem_pair` of tests/test_gpu_stem.py does); kink-free parameters add 8 to every norm bias, so that no pre-activation is near
zero and no ReLU mask can differ between two precisions.  With ordinary parameters a pre-activation within rounding of zero has a
different mask in different precisions and moves a gradient by O(1) of one element, so a row's SEED is recorded by the rule of
tests/stem_geometry_cases.py, which reads two CPU runs only: over the GroupNorm outputs u of the float64 run,
min |u| / (8 x the max-abs distance of the float32 CPU run's u from the float64 one, per tensor) >= 1.  The recorded seed is the
first of 1 ... 200 whose margin is at least SEARCHED_MARGIN (2: room for hosts whose fp32 kernels differ, as that file explains).
The number of tries grows as exp(margin x 4e-6 x the number of pre-activations), and the four shapes of 0.6 - 1.3 million
pre-activations have no such seed among 200 (best margins 0.3 - 0.5): three of them keep the FIRST seed at all that meets the rule
as stated (1115, 4901 and 10725 tries), the fourth is RELATIVE_L2.  The host test asserts the rule as stated, margin >= 1, for every
seed recorded under it.  `python -m tests.stem_banded_cases [name ...]` searches."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> (n, in_ch, h, w, filters)
SHAPES = {
    's51_f64': (1, 3, 51, 51, 64),            # 49 x 49 = 2401 px: the first shape past the resident passes' ceiling
    's64_f128': (2, 3, 64, 64, 128),          # tiny-imagenet-200's images
    's64_f1024': (2, 3, 64, 64, 1024),        # the filters of BASELINE.json configs[4]: 32 channels per group at the last norm
    'r53x70_in1': (3, 1, 53, 70, 64),         # rectangular, one input channel, odd batch, 51 x 68 = 3468 = 27 x 128 + 12: a short last band
    's102_f64': (1, 3, 102, 102, 64),         # 100 x 100, then 50 x 50 = 2500: three banded norms, the triples-writing backward
    # the Python gate sends these two to the resident node: run through the ABI under NODE_TUNE_STEM_BANDED=all, NODE_TUNE_STEM_BAND_PX=16
    's32_f256': (2, 3, 32, 32, 256),          # every norm banded; 8 channels per group at the last one; 900 = 56 x 16 + 4
    'r9x12_in1': (2, 1, 9, 12, 64),           # 7 x 10 = 70 px (five bands, the last of 6), then 4 x 5 and 2 x 3: one band shorter than a lane group
}
GATE = ('s51_f64', 's64_f128', 's64_f1024', 'r53x70_in1', 's102_f64')     # what ResidualStem.forward sends to _BandedStemFn
ABI_ONLY = ('s32_f256', 'r9x12_in1')
ALL_ENV = {'NODE_TUNE_STEM_BANDED': 'all', 'NODE_TUNE_STEM_BAND_PX': '16'}
SEARCHED_MARGIN = 2
# the seeds the rule gives, with the margin they had where they were searched
SEEDS = {
    's51_f64': 100,          # 2.35
    's32_f256': 1,           # 2.35
    'r9x12_in1': 1,          # 3.08
    's64_f128': 4901,        # 1.04
    's102_f64': 10725,       # 1.11
    'r53x70_in1': 1115,      # 1.34
    's64_f1024': 1027,       # no seed of 1 ... 200 meets the rule (best 0.33): `_stem_pair`'s own, in_ch + filters; see RELATIVE_L2
}
# the one shape held to the relative-L2 bound 2e-2 on its gradients with ordinary parameters (its output and its kink-free run keep the
# max-norm bound): 1.26 million pre-activations at 0.5 s a try -- the ~40 000 tries the other large shapes' margins suggest were not run
RELATIVE_L2 = ('s64_f1024',)


def build(name, seed=None, kink_free=False):
    """(fp32 stem on the CPU, input, cotangent) of a shape: parameters from `seed` (default: the recorded one)."""
    import torch
    import neural_ode_features_amd as nof
    n, in_ch, h, w, filters = SHAPES[name]
    seed = SEEDS[name] if seed is None else seed
    torch.manual_seed(seed)
    stem = nof.ODENet(in_ch, out=10, n_filters=filters, downsample='residual', adjoint=True).downsample.module
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for pname, p in stem.named_parameters():
            if 'norm' in pname:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if kink_free and pname.endswith('bias'):
                    p.add_(8.0)
    x = torch.randn(n, in_ch, h, w, generator=gen)
    with torch.no_grad():
        shape = stem(x).shape
    cot = torch.randn(shape, generator=gen)
    return stem, x, cot


def seed_margin(name, seed=None):
    """min |u| / (8 x the fp32 CPU run's distance) over the GroupNorm outputs of the float64 run: the seed rule holds where this is >= 1"""
    import torch
    from neural_ode_features_amd import stem as S
    from tests import stem_geometry_cases as G
    mod, x, cot = build(name, seed)
    return G.margin_of(G.cpu_run(mod, S._params_of, x, cot, torch.float64, False), G.cpu_run(mod, S._params_of, x, cot, torch.float32, False))


_REFS = {}


def reference(name, kink_free):
    """{'inputs': (stem, x, cot), 'ref': the float64 run of the modules on the CPU (tests/stem_geometry_cases.cpu_run)}: computed once
    per process, never changed."""
    import torch
    from neural_ode_features_amd import stem as S
    from tests import stem_geometry_cases as G
    key = (name, bool(kink_free))
    if key not in _REFS:
        mod, x, cot = build(name, kink_free=kink_free)
        _REFS[key] = {'inputs': (mod, x, cot), 'ref': G.cpu_run(mod, S._params_of, x, cot, torch.float64)}
    return _REFS[key]


def _search(job):
    import torch
    torch.set_num_threads(1)
    name, seed = job
    return name, seed, seed_margin(name, seed)


if __name__ == '__main__':
    import multiprocessing as mp
    names = sys.argv[1:] or list(SHAPES)
    workers = min(16, os.cpu_count() or 1)
    with mp.get_context('spawn').Pool(workers) as pool:
        for name in names:
            # the first of 1 ... 200 with the searched margin; failing that, the first seed at all that meets the rule as stated
            lo, found, first_ok = 1, None, None
            while found is None and lo < 200000 and not (first_ok and lo > 200):
                got = pool.map(_search, [(name, s) for s in range(lo, lo + 8 * workers)])
                ok = [(s, m) for _, s, m in got if m >= SEARCHED_MARGIN and s <= 200]
                if first_ok is None and any(m >= 1 for _, s, m in got):
                    first_ok = min((s, m) for _, s, m in got if m >= 1)
                if ok:
                    found = min(ok)
                lo += 8 * workers
            found = found or first_ok
            print("    %r: %s,      # %s" % (name, found[0] if found else None, ('%.2f' % found[1]) if found else 'none'), flush=True)

"""Cases, parameters and fp64 references shared by tests/test_bnconvstem_host.py, tests/test_gpu_bnconvstem.py and
tests/test_gpu_bndownconv.py: the `norm='batch'` convolution stem (model.py:148-164 with model.py:274) as one HIP node
(convstem.py `_BnConvStemFn`, csrc/bnconvstem_api.hip), the `ode2` stem's hand-off `conv2(norm(x))` (model.py:199-223) as another
(downconv.py `_BnDownConvFn`, csrc/bndownconv_api.hip), and that hand-off on a whole trajectory, slice by slice (model.py:214-216).

Three families of cases, every one a small `nn.Module` whose reference is the same modules as `.double()` on the CPU, run as module
operations (`nn.Sequential.forward`), never the node:
    'stem'    (in_ch, side, F, N): `nof.ODENet(in_ch, out=10, n_filters=F, downsample='convolution', adjoint=True,
              norm='batch').downsample.module` after `torch.manual_seed(seed)`
    'down'    (N, cin, cout, side): `nn.Sequential(BatchNorm2d(cin, track_running_stats=False), ReLU(), Conv2d(cin, cout, 4, 2, 1))`
              after `torch.manual_seed(seed)`; the node takes [0] and [2] as parameter containers
    'sliced'  (T, N, C, side): the 'down' modules at cin = cout = C on an input [T, N, C, H, W], the reference slice by slice; slice k
              of the input is scaled by 1 + k / 2 and shifted by 0.3 k, so that no two slices share their statistics

Metric, bound, parameter sets and seed recipe are tests/bnstem_cases.py's, unchanged: bntrunk_cases.errors; per quantity
max(2e-5, 4 x the error of the fp32 modules on the CPU against fp64); norm weights and biases perturbed by 0.2 randn from
Generator(seed + 1) ('ordinary'), and +8 ('kinkfree') or +8 / -8 by channel parity ('split') on the norms' biases (each sits in
front of a ReLU); the input is randn from Generator(seed + 2), the cotangent drawn from the same generator behind it.  A seed of an
ordinary run is admitted only if (a) every ReLU mask agrees between the fp32 and the fp64 CPU run and (b) its margin ratio --
smallest |pre-activation| of the fp64 run over the largest error of an fp32 pre-activation -- is at least
bnfunc_cases.RATIO_YARDSTICK's (2.60).  Seeds 0..19 are searched first, 0..199 if none of them is admissible; among the admissible
seeds the one with the largest margin is kept (`python tests/bnconvstem_cases.py` prints the table).  A case without an entry in
SEEDS has no admissible seed and runs kink-free and split only."""
import copy
import functools
import os
import sys

import torch
from torch import nn

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bnfunc_cases as B  # noqa: E402
from tests import bnstem_cases as S  # noqa: E402

MODES = B.MODES
KINK_FREE_SEED = B.KINK_FREE_SEED
REGIMES = S.REGIMES
bound = S.bound

# ('stem', in_ch, side, F, N); side: H = W, or (H, W) -- the smallest shapes at which each part of the plan can go wrong
STEM_CASES = [('stem', 1, 28, 64, 2),          # MNIST geometry: 26 -> 13 -> 6, odd sizes in the parity classes
              ('stem', 3, 32, 128, 3),         # two column tiles behind the last convolution, odd batch
              ('stem', 3, 32, 256, 2),         # the CIFAR width
              ('stem', 3, 32, 192, 2),         # three column tiles, not a power of two: the GroupNorm stem refuses it
              ('stem', 3, (12, 10), 64, 2),    # H != W: 10 x 8 -> 5 x 4 -> 2 x 2
              ('stem', 1, 10, 64, 1)]          # the floor: four values per channel behind the last convolution, batch 1
# the launch regimes STEM_CASES does not reach, asked of the norm named by its index 0..1: under the default cap of 128 chunks,
# 4 500 rows in 71 chunks of 64 (two trips), the last of 20 rows; 1 125 rows in 36 chunks of 32, the last of 5
STEM_MULTI = {('stem', 3, 32, 64, 5): ((0, 'several_chunks'), (0, 'two_trips'), (0, 'short_last_chunk'), (1, 'several_chunks'))}
STEM_ALL = STEM_CASES + list(STEM_MULTI)
# ('down', N, cin, cout, side)
DOWN_CASES = [('down', 2, 64, 64, 4),          # the floor: 32 rows, 2 x 2 out
              ('down', 2, 64, 64, (7, 6)),     # odd sizes: 84 rows, 3 x 3 out
              ('down', 3, 128, 128, 8),
              ('down', 2, 256, 256, 16),
              ('down', 2, 192, 192, 8),        # three column tiles both ways: the GroupNorm hand-off refuses it
              ('down', 2, 64, 128, 8)]         # cin != cout
# 9 x 24 x 19 = 4 104 rows at C = 64: 65 chunks of 64 rows (two 32-row trips each), the last of 8 rows
DOWN_MULTI = {('down', 9, 64, 64, (24, 19)): ('several_chunks', 'two_trips', 'short_last_chunk')}
DOWN_ALL = DOWN_CASES + list(DOWN_MULTI)
# ('sliced', T, N, C, side): 128 rows per slice in four whole chunks; 84 rows per slice -- chunks start at rows 84, 116, 148, 168, ..,
# off every 32-row boundary, and every slice ends in a chunk of 20 rows
SLICED_CASES = [('sliced', 3, 2, 64, 8), ('sliced', 3, 2, 64, (7, 6))]
ALL_CASES = STEM_ALL + DOWN_ALL + SLICED_CASES

# chosen by the recipe of the docstring (`python tests/bnconvstem_cases.py`); the table it printed (the yardstick stands at 2.60):
#     ('stem', 1, 28, 64, 2) seeds 0..19: 20 with equal masks, 12 admissible -> kept 5, smallest |pre-activation| 3.29e-05, margin / error 15.49
#     ('stem', 3, 32, 128, 3) seeds 0..19: 20 with equal masks, 5 admissible -> kept 15, smallest |pre-activation| 2.06e-05, margin / error 11.71
#     ('stem', 3, 32, 256, 2) seeds 0..19: 20 with equal masks, 12 admissible -> kept 17, smallest |pre-activation| 6.60e-05, margin / error 37.92
#     ('stem', 3, 32, 192, 2) seeds 0..19: 20 with equal masks, 12 admissible -> kept 17, smallest |pre-activation| 6.60e-05, margin / error 37.92
#     ('stem', 3, (12, 10), 64, 2) seeds 0..19: 20 with equal masks, 20 admissible -> kept 18, smallest |pre-activation| 2.94e-04, margin / error 202.00
#     ('stem', 1, 10, 64, 1) seeds 0..19: 20 with equal masks, 20 admissible -> kept 2, smallest |pre-activation| 9.45e-04, margin / error 718.22
#     ('stem', 3, 32, 64, 5) seeds 0..19: 20 with equal masks, 6 admissible -> kept 0, smallest |pre-activation| 1.22e-05, margin / error 6.63
#     ('down', 2, 64, 64, 4) seeds 0..19: 20 with equal masks, 20 admissible -> kept 9, smallest |pre-activation| 1.67e-03, margin / error 6234.28
#     ('down', 2, 64, 64, (7, 6)) seeds 0..19: 20 with equal masks, 20 admissible -> kept 4, smallest |pre-activation| 5.98e-04, margin / error 1098.79
#     ('down', 3, 128, 128, 8) seeds 0..19: 20 with equal masks, 20 admissible -> kept 6, smallest |pre-activation| 2.03e-04, margin / error 445.53
#     ('down', 2, 256, 256, 16) seeds 0..19: 20 with equal masks, 18 admissible -> kept 18, smallest |pre-activation| 2.55e-05, margin / error 41.89
#     ('down', 2, 192, 192, 8) seeds 0..19: 20 with equal masks, 20 admissible -> kept 19, smallest |pre-activation| 2.11e-04, margin / error 309.06
#     ('down', 2, 64, 128, 8) seeds 0..19: 20 with equal masks, 20 admissible -> kept 2, smallest |pre-activation| 4.34e-04, margin / error 1147.75
#     ('down', 9, 64, 64, (24, 19)) seeds 0..19: 20 with equal masks, 18 admissible -> kept 11, smallest |pre-activation| 1.34e-05, margin / error 23.67
#     ('sliced', 3, 2, 64, 8) seeds 0..19: 20 with equal masks, 20 admissible -> kept 14, smallest |pre-activation| 1.46e-04, margin / error 350.22
#     ('sliced', 3, 2, 64, (7, 6)) seeds 0..19: 20 with equal masks, 20 admissible -> kept 13, smallest |pre-activation| 1.90e-04, margin / error 424.12
# (the stem's pre-activations do not depend on F: the two rows at F = 256 and 192 are one search.)  The one-sign-per-channel condition
# of 'kinkfree' and 'split' holds in fp64 for all sixteen cases with KINK_FREE_SEED; the smallest |pre-activation| is 0.81, at the stems
# of 32 x 32 images kink-free.  The whole model: 15 norms, one sign per channel, 0.91 / 1.65.
SEEDS = {('stem', 1, 28, 64, 2): 5, ('stem', 3, 32, 128, 3): 15, ('stem', 3, 32, 256, 2): 17, ('stem', 3, 32, 192, 2): 17,
         ('stem', 3, (12, 10), 64, 2): 18, ('stem', 1, 10, 64, 1): 2, ('stem', 3, 32, 64, 5): 0,
         ('down', 2, 64, 64, 4): 9, ('down', 2, 64, 64, (7, 6)): 4, ('down', 3, 128, 128, 8): 6, ('down', 2, 256, 256, 16): 18,
         ('down', 2, 192, 192, 8): 19, ('down', 2, 64, 128, 8): 2, ('down', 9, 64, 64, (24, 19)): 11,
         ('sliced', 3, 2, 64, 8): 14, ('sliced', 3, 2, 64, (7, 6)): 13}


def _hw(side):
    return side if isinstance(side, tuple) else (side, side)


def _out4(h):
    return (h + 2 - 4) // 2 + 1


def shape_of(case):
    """the input's shape"""
    kind = case[0]
    if kind == 'stem':
        _, cin, side, _, n = case
        return (n, cin) + _hw(side)
    if kind == 'down':
        _, n, cin, _, side = case
        return (n, cin) + _hw(side)
    _, t, n, c, side = case
    return (t, n, c) + _hw(side)


def out_shape_of(case):
    kind = case[0]
    s = shape_of(case)
    if kind == 'stem':
        return (s[0], case[3], _out4(_out4(s[2] - 2)), _out4(_out4(s[3] - 2)))
    if kind == 'down':
        return (s[0], case[3], _out4(s[2]), _out4(s[3]))
    return (s[0], s[1], s[2], _out4(s[3]), _out4(s[4]))


def norm_names(case):
    """the state_dict prefixes of the case's norms"""
    return ('1.', '4.') if case[0] == 'stem' else ('0.',)


def norms_of(mod):
    return [m for m in mod if isinstance(m, nn.BatchNorm2d)]


def module_pair(case, seed, mode='ordinary'):
    """(the fp32 modules of a case, their fp64 copy)"""
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    if case[0] == 'stem':
        mod = nof.ODENet(case[1], out=10, n_filters=case[3], downsample='convolution', adjoint=True, norm='batch').downsample.module
    else:
        cin, cout = (case[2], case[3]) if case[0] == 'down' else (case[3], case[3])
        mod = nn.Sequential(nn.BatchNorm2d(cin, track_running_stats=False), nn.ReLU(), nn.Conv2d(cin, cout, 4, 2, 1))
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.startswith(norm_names(case)):
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if name.endswith('.bias'):
                    if mode == 'kinkfree':
                        p.add_(8.0)
                    elif mode == 'split':
                        p[0::2] += 8.0
                        p[1::2] -= 8.0
    return mod, copy.deepcopy(mod).double()


def case_inputs(case, seed):
    """(x, cotangent) of a case"""
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(*shape_of(case), generator=gen)
    cot = torch.randn(*out_shape_of(case), generator=gen)
    if case[0] == 'sliced':          # slice k scaled by 1 + k / 2 and shifted by 0.3 k: no two slices share their statistics
        k = torch.arange(x.shape[0], dtype=x.dtype).reshape(-1, 1, 1, 1, 1)
        x = x * (1.0 + 0.5 * k) + 0.3 * k
    return x, cot


def modules_forward(mod, x):
    """the module operations: nn.Sequential.forward, slice by slice for a trajectory"""
    if x.dim() == 5:
        return torch.stack([nn.Sequential.forward(mod, xi) for xi in x])
    return nn.Sequential.forward(mod, x)


def preactivations(mod, x):
    """the outputs of the norms of a CPU run of the module operations (a trajectory: one per slice)"""
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())) for m in norms_of(mod)]
    with torch.no_grad():
        modules_forward(mod, x)
    for h in hooks:
        h.remove()
    return outs


@functools.lru_cache(maxsize=None)
def margin_ratio(case, seed):
    """Ordinary parameters: (every ReLU mask of the fp32 and the fp64 CPU run agrees, margin = the smallest |pre-activation| of
    the fp64 run, margin / the largest |fp32 pre-activation - fp64 pre-activation|)"""
    mod, ref = module_pair(case, seed)
    x, _ = case_inputs(case, seed)
    p32, p64 = preactivations(mod, x), preactivations(ref, x.double())
    assert len(p64) == (2 if case[0] == 'stem' else 1 if case[0] == 'down' else case[1])
    agree = all(torch.equal(a > 0, b > 0) for a, b in zip(p32, p64))
    margin = min(float(b.abs().min()) for b in p64)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    return agree, margin, margin / err


def sign_condition(case, mode):
    """The fp64 CPU run of a 'kinkfree' or 'split' set: (every channel of every norm's output has one sign over all rows, the
    smallest |pre-activation|)"""
    _, ref = module_pair(case, KINK_FREE_SEED, mode)
    x, _ = case_inputs(case, KINK_FREE_SEED)
    constant, margin = True, float('inf')
    for o in preactivations(ref, x.double()):
        pos = (o > 0).permute(1, 0, 2, 3).reshape(o.shape[1], -1)
        constant = constant and bool((pos.all(dim=1) | (~pos).all(dim=1)).all())
        margin = min(margin, float(o.abs().min()))
    return constant, margin


def seed_of(case, mode):
    return SEEDS[case] if mode == 'ordinary' else KINK_FREE_SEED


def runs(case):
    """the (case, mode) pairs a case runs: 'ordinary' only with an admitted seed"""
    return [(case, m) for m in MODES if m != 'ordinary' or case in SEEDS]


def run_modules(mod, x, cot, forward=None):
    """Forward + backward: (out, d_x, parameter gradients by name, ()).  `forward`: how to call the modules (default: the module
    operations, `modules_forward`)."""
    xg = x.clone().requires_grad_(True)
    for p in mod.parameters():
        p.grad = None
    out = (forward or modules_forward)(mod, xg)
    out.backward(cot)
    return out.detach(), xg.grad, {k: p.grad.clone() for k, p in mod.named_parameters()}, ()


@functools.lru_cache(maxsize=None)
def references(case, mode):
    """Computed once and shared, never modified: (the fp64 CPU run, the fp32 CPU run of the module operations), each as
    `run_modules` returns it.  The fp32 run is what the second term of the bounds is taken from."""
    seed = seed_of(case, mode)
    mod, ref = module_pair(case, seed, mode)
    x, cot = case_inputs(case, seed)
    return run_modules(ref, x.double(), cot.double()), run_modules(mod, x, cot)


# ---------------------------------------------------------------------------------------------------------------------
# The whole model: ResNet(3, n_filters=64, downsample='convolution', norm='batch') at [4, 3, 32, 32] -- this stem (32 -> 30 -> 15 -> 7),
# six blocks at 7 x 7, the BatchNorm head.  Kink-free and split only, with KINK_FREE_SEED, as tests/bntrunk_cases.py runs its model.
# ---------------------------------------------------------------------------------------------------------------------
MODEL_SHAPE = (4, 3, 32, 32)
MODEL_MODES = ('kinkfree', 'split')
MODEL_BLOCKS = 6


def model_pair(seed, mode):
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    net = nof.ResNet(3, n_filters=64, downsample='convolution', norm='batch')
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if 'norm' in name or name.startswith(('classifier.module.0.', 'downsample.module.1.', 'downsample.module.4.')):
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if name.endswith('.bias'):
                    if mode == 'kinkfree':
                        p.add_(8.0)
                    elif mode == 'split':
                        p[0::2] += 8.0
                        p[1::2] -= 8.0
    return net, copy.deepcopy(net).double()


def model_inputs(seed):
    gen = torch.Generator().manual_seed(seed + 2)
    return torch.randn(*MODEL_SHAPE, generator=gen), torch.randn(MODEL_SHAPE[0], 10, generator=gen)


def model_sign_condition(mode):
    """the fp64 CPU run of the whole model: (norms, one sign per channel of every BatchNorm output, the smallest |pre-activation|)"""
    _, ref = model_pair(KINK_FREE_SEED, mode)
    x, _ = model_inputs(KINK_FREE_SEED)
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())) for m in ref.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        ref(x.double())
    for h in hooks:
        h.remove()
    constant, margin = True, float('inf')
    for o in outs:
        pos = (o > 0).permute(1, 0, 2, 3).reshape(o.shape[1], -1)
        constant = constant and bool((pos.all(dim=1) | (~pos).all(dim=1)).all())
        margin = min(margin, float(o.abs().min()))
    return len(outs), constant, margin


@functools.lru_cache(maxsize=None)
def model_references(mode):
    """(the fp64 CPU run, the fp32 CPU run) of the whole model, each as bntrunk_cases.run_model returns it"""
    from tests import bntrunk_cases as T
    net, ref = model_pair(KINK_FREE_SEED, mode)
    x, cot = model_inputs(KINK_FREE_SEED)
    return T.run_model(ref, x.double(), cot.double()), T.run_model(net, x, cot)


if __name__ == '__main__':      # the seed table (CPU only)
    need = B.margin_ratio(*B.RATIO_YARDSTICK)[2]
    print('yardstick %s seed %d: margin / error %.2f' % (B.RATIO_YARDSTICK + (need,)))
    for case in ALL_CASES:
        for top in (20, 200):
            rows = [(s,) + margin_ratio(case, s) for s in range(top)]
            ok = [(m, s, r) for s, agree, m, r in rows if agree and r >= need]
            if ok:
                break
        best = max(rows, key=lambda r: r[3])
        eligible = sum(1 for r in rows if r[1])
        if ok:
            print(case, 'seeds 0..%d: %d with equal masks, %d admissible -> kept %d, smallest |pre-activation| %.2e, margin / error %.2f'
                  % (top - 1, eligible, len(ok), max(ok)[1], max(ok)[0], max(ok)[2]), flush=True)
        else:
            print(case, 'seeds 0..%d: %d with equal masks, none admissible (best margin / error %.2f at seed %d): kink-free and split only'
                  % (top - 1, eligible, best[3], best[0]), flush=True)
    for case in ALL_CASES:
        for mode in ('kinkfree', 'split'):
            print(case, mode, 'one sign per channel: %s, smallest |pre-activation| %.2f' % sign_condition(case, mode), flush=True)
    for mode in MODEL_MODES:
        print('model', mode, '%d norms, one sign per channel: %s, smallest |pre-activation| %.2f' % model_sign_condition(mode), flush=True)

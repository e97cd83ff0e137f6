"""Cases, parameters and fp64 references shared by tests/test_bnministem_host.py and tests/test_gpu_bnministem.py: the `norm='batch'`
minimal stem (model.py:129-145 with model.py:274) as one HIP node (ministem.py `_BnMiniStemFn`, csrc/bnministem_api.hip).  It is
tests/bnconvstem_cases.py's 'stem' family with downsample='minimal'.

A case (in_ch, side, F, N) is `nof.ODENet(in_ch, out=10, n_filters=F, downsample='minimal', adjoint=True, norm='batch')
.downsample.module` after `torch.manual_seed(seed)`; its reference is the same modules as `.double()` on the CPU, run as module
operations (`nn.Sequential.forward`), never the node.

Metric, bound, parameter sets and seed recipe are tests/bnstem_cases.py's, unchanged: bntrunk_cases.errors; per quantity
max(2e-5, 4 x the error of the fp32 modules on the CPU against fp64); norm weights and biases ('1.', '4.') perturbed by 0.2 randn
from Generator(seed + 1) ('ordinary'), and +8 ('kinkfree') or +8 / -8 by channel parity ('split') on the norms' biases (each sits in
front of a ReLU); the input is randn from Generator(seed + 2), the cotangent drawn from the same generator behind it.  A seed of an
ordinary run is admitted only if (a) every ReLU mask agrees between the fp32 and the fp64 CPU run and (b) its margin ratio --
smallest |pre-activation| of the fp64 run over the largest error of an fp32 pre-activation -- is at least
bnfunc_cases.RATIO_YARDSTICK's (2.60).  Seeds 0..19 are searched first, 0..199 if none of them is admissible; among the admissible
seeds the one with the largest margin is kept (`python tests/bnministem_cases.py` prints the table).  A case without an entry in
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
from tests import bntrunk_cases as T  # noqa: E402

MODES = B.MODES
KINK_FREE_SEED = B.KINK_FREE_SEED
RATIO_YARDSTICK = B.RATIO_YARDSTICK
bound = S.bound
errors, model_errors, run_model, model_bound = T.errors, T.model_errors, T.run_model, T.bound

# (in_ch, side, F, N); side: H = W, or (H, W) -- the smallest shapes at which each part of the plan can go wrong
CASES = [(1, 28, 64, 2),          # MNIST geometry: 26 -> 13 -> 6, odd sizes
         (3, 32, 128, 3),         # odd batch
         (3, 32, 256, 2),         # the CIFAR width
         (3, (12, 10), 64, 2),    # H != W: 10 x 8 -> 5 x 4 -> 2 x 2
         (1, 10, 64, 1)]          # the floor, batch 1: 16 values per channel at the second norm
# The launch regimes of the BatchNorm passes, defined on the fields of node_bnministem_info (`_lib.bnministem_plan`): a workgroup per
# chunk of chunk_rows rows, walked trip_rows rows at a time.
REGIMES = {
    'several_chunks': lambda d: d['nchunk'] > 4,
    'several_trips': lambda d: d['chunk_rows'] > d['trip_rows'],
    'short_last_chunk': lambda d: d['last_chunk_rows'] < d['trip_rows'],
    'single_chunk': lambda d: d['nchunk'] == 1 and d['last_chunk_rows'] == d['rows'],
}
# (case) -> ((norm 0..1, regime), ..).  Under the cap of 128 chunks and trips of 32 rows: (3, 32, 64, 5) has 4 500 rows in 71 chunks of
# 64 (two trips), the last of 20 rows, and 1 125 rows in 36 chunks of 32, the last of 5; (1, 10, 64, 1) has 64 rows in two whole chunks
# and 16 rows in ONE chunk.
MULTI = {(3, 32, 64, 5): ((0, 'several_chunks'), (0, 'several_trips'), (0, 'short_last_chunk'), (1, 'several_chunks'),
                          (1, 'short_last_chunk')),
         (1, 10, 64, 1): ((1, 'single_chunk'), (1, 'short_last_chunk'))}
ALL_CASES = CASES + [c for c in MULTI if c not in CASES]

# chosen by the recipe of the docstring (`python tests/bnministem_cases.py`); the table it printed (the yardstick stands at 2.60):
#     (1, 28, 64, 2) seeds 0..19: 20 with equal masks, 15 admissible -> kept 14, smallest |pre-activation| 6.48e-05, margin / error 35.70
#     (3, 32, 128, 3) seeds 0..19: 20 with equal masks, 14 admissible -> kept 10, smallest |pre-activation| 3.43e-05, margin / error 17.71
#     (3, 32, 256, 2) seeds 0..19: 20 with equal masks, 17 admissible -> kept 9, smallest |pre-activation| 8.43e-05, margin / error 51.64
#     (3, (12, 10), 64, 2) seeds 0..19: 20 with equal masks, 20 admissible -> kept 13, smallest |pre-activation| 7.31e-04, margin / error 722.38
#     (1, 10, 64, 1) seeds 0..19: 20 with equal masks, 19 admissible -> kept 3, smallest |pre-activation| 1.93e-03, margin / error 2230.32
#     (3, 32, 64, 5) seeds 0..19: 20 with equal masks, 10 admissible -> kept 16, smallest |pre-activation| 3.20e-05, margin / error 15.50
# The one-sign-per-channel condition of 'kinkfree' and 'split' holds in fp64 for all six cases with KINK_FREE_SEED; the smallest
# |pre-activation| is 1.85, at (3, 32, 64, 5) kink-free.  The whole model: 15 norms, one sign per channel, 2.10 / 2.60; the fp32 modules
# on the CPU stand at 7.2e-5 / 7.3e-5 at their worst, a trunk convolution's weight gradient.
SEEDS = {(1, 28, 64, 2): 14, (3, 32, 128, 3): 10, (3, 32, 256, 2): 9, (3, (12, 10), 64, 2): 13, (1, 10, 64, 1): 3, (3, 32, 64, 5): 16}


def _hw(side):
    return side if isinstance(side, tuple) else (side, side)


def _out4(h):
    return (h + 2 - 4) // 2 + 1


def shape_of(case):
    """the input's shape"""
    cin, side, _, n = case
    return (n, cin) + _hw(side)


def out_shape_of(case):
    s = shape_of(case)
    return (s[0], case[2], _out4(_out4(s[2] - 2)), _out4(_out4(s[3] - 2)))


NORM_NAMES = ('1.', '4.')       # the state_dict prefixes of the stem's norms


def plan_of(case):
    from neural_ode_features_amd import _lib
    n, cin, h, w = shape_of(case)
    return _lib.bnministem_plan(n, cin, h, w, case[2])


def module_pair(case, seed, mode='ordinary'):
    """(the fp32 modules of a case, their fp64 copy)"""
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    mod = nof.ODENet(case[0], out=10, n_filters=case[2], downsample='minimal', adjoint=True, norm='batch').downsample.module
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.startswith(NORM_NAMES):
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
    return x, cot


def modules_forward(mod, x):
    """the module operations"""
    return nn.Sequential.forward(mod, x)


def preactivations(mod, x):
    """the outputs of the norms of a CPU run of the module operations"""
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())) for m in mod if isinstance(m, nn.BatchNorm2d)]
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
    assert len(p64) == 2
    agree = all(torch.equal(a > 0, b > 0) for a, b in zip(p32, p64))
    margin = min(float(b.abs().min()) for b in p64)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    return agree, margin, margin / err


def _one_sign(outs):
    constant, margin = True, float('inf')
    for o in outs:
        pos = (o > 0).permute(1, 0, 2, 3).reshape(o.shape[1], -1)
        constant = constant and bool((pos.all(dim=1) | (~pos).all(dim=1)).all())
        margin = min(margin, float(o.abs().min()))
    return constant, margin


def sign_condition(case, mode):
    """The fp64 CPU run of a 'kinkfree' or 'split' set: (every channel of every norm's output has one sign over all rows, the
    smallest |pre-activation|)"""
    _, ref = module_pair(case, KINK_FREE_SEED, mode)
    x, _ = case_inputs(case, KINK_FREE_SEED)
    return _one_sign(preactivations(ref, x.double()))


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
# The whole model: ResNet(3, n_filters=64, downsample='minimal', norm='batch') at [4, 3, 32, 32] -- this stem (32 -> 30 -> 15 -> 7),
# six blocks at 7 x 7, the BatchNorm head.  Kink-free and split only, with KINK_FREE_SEED, as tests/bntrunk_cases.py runs its model.
# ---------------------------------------------------------------------------------------------------------------------
MODEL_SHAPE = (4, 3, 32, 32)
MODEL_MODES = ('kinkfree', 'split')
MODEL_BLOCKS = 6


def model_pair(seed, mode):
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    net = nof.ResNet(3, n_filters=64, downsample='minimal', norm='batch')
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
    return (len(outs),) + _one_sign(outs)


@functools.lru_cache(maxsize=None)
def model_references(mode):
    """(the fp64 CPU run, the fp32 CPU run) of the whole model, each as bntrunk_cases.run_model returns it"""
    net, ref = model_pair(KINK_FREE_SEED, mode)
    x, cot = model_inputs(KINK_FREE_SEED)
    return run_model(ref, x.double(), cot.double()), run_model(net, x, cot)


if __name__ == '__main__':      # the seed table (CPU only)
    need = B.margin_ratio(*RATIO_YARDSTICK)[2]
    print('yardstick %s seed %d: margin / error %.2f' % (RATIO_YARDSTICK + (need,)))
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
    for mode in MODEL_MODES:
        r64, r32 = model_references(mode)
        floor = model_errors(r32, r64)
        worst = max(floor, key=floor.get)
        print('model', mode, 'fp32 modules on the CPU: worst error %.1e at %s' % (floor[worst], worst), flush=True)

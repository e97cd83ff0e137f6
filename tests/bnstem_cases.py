"""Cases, parameters and fp64 references shared by tests/test_bnstem_host.py and tests/test_gpu_bnstem.py: the `norm='batch'`
residual stem (model.py:167-178 of ResBlocks model.py:284-310 with model.py:274) as one HIP node (stem.py `_BnStemFn`,
csrc/bnstem_api.hip).

The stem of a case is `nof.ODENet(in_ch, out=10, n_filters=F, downsample='residual', adjoint=True, norm='batch').downsample.module`
after `torch.manual_seed(seed)`.  The reference of every comparison is the same modules as `.double()` on the CPU, run as
`nn.Sequential.forward`: the module operations, never the node.

Parameter sets follow tests/bntrunk_cases.py: norm weights and biases perturbed by 0.2 randn from Generator(seed + 1) ('ordinary'),
and +8 ('kinkfree') or +8 / -8 by channel parity ('split') on the biases of all four norms (each sits in front of a ReLU).  The
input is randn from Generator(seed + 2), the cotangent is drawn from the same generator behind it.

Seeds of the ordinary runs follow that file's recipe (`python tests/bnstem_cases.py` prints the table): the module operations run
in fp32 and in fp64 on the CPU, and a seed is admitted only if (a) EVERY ReLU mask (the sign of every output of the four norms)
agrees between the two and (b) its margin ratio -- smallest |pre-activation| of the fp64 run over the largest error of an fp32
pre-activation -- is at least bnfunc_cases.RATIO_YARDSTICK's (2.60).  Seeds 0..19 are searched first, 0..199 if none of them is
admissible; among the admissible seeds the one with the largest margin is kept.  A case without an entry in SEEDS has no
admissible seed and runs kink-free and split only."""
import copy
import functools
import os
import sys

import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bnfunc_cases as B  # noqa: E402

MODES = B.MODES
KINK_FREE_SEED = B.KINK_FREE_SEED
# (in_ch, side, F, N); side: H = W, or (H, W) -- the smallest shapes at which each part of the plan can go wrong
CASES = [(1, 28, 64, 2),          # MNIST geometry: 26 -> 13 -> 7, 98 rows at the last norm (ragged 32-row trip, odd sizes in every parity class)
         (3, 32, 128, 3),         # two column tiles in block 2, odd batch
         (3, 32, 256, 2),         # the CIFAR width
         (3, 32, 192, 2),         # three column tiles, not a power of two: the GroupNorm stem refuses it
         (3, (12, 9), 64, 2),     # H != W: 10 x 7 -> 5 x 4 -> 3 x 2
         (1, (6, 5), 64, 4)]      # the floor: 4 x 3 -> 2 x 2 -> 1 x 1, four values per channel at the last norm
# the launch regimes CASES does not reach (REGIMES of bnfunc_cases.py, asked of the norm named by its index 0..3; 'eight_trips' and
# 'one_row_last_chunk' are defined below): under the default cap of 128 chunks
#     (3, 32, 64, 5):   4 500 rows in 71 chunks of 64, the last of 20 rows; 1 125 rows in 36 chunks of 32, the last of 5
#     (3, 32, 64, 33): 29 700 rows in 117 chunks of 256 (eight trips), the last of 4 rows; 7 425 rows in 117 chunks of 64, the last of ONE
REGIMES = dict(B.REGIMES)
REGIMES['eight_trips'] = lambda d: d['chunk_rows'] == 256
REGIMES['one_row_last_chunk'] = lambda d: d['chunk_rows'] > 32 and d['last_chunk_rows'] == 1
MULTI_CASES = {
    (3, 32, 64, 5): ((0, 'several_chunks'), (0, 'two_trips'), (0, 'short_last_chunk'), (1, 'several_chunks')),
    (3, 32, 64, 33): ((0, 'several_chunks'), (0, 'eight_trips'), (0, 'short_last_chunk'), (1, 'two_trips'), (1, 'one_row_last_chunk'),
                      (2, 'one_row_last_chunk'), (3, 'several_chunks')),
}
ALL_CASES = CASES + list(MULTI_CASES)
# chosen by the recipe of the docstring (`python tests/bnstem_cases.py`); the table it printed (the yardstick stands at 2.60):
# seeds searched / with equal masks / admissible / kept / smallest |pre-activation| / margin over error
#     (1, 28, 64, 2)       0..19 / 19 / 10 /  5 / 3.3e-5 / 15.5      (3, (12, 9), 64, 2)  0..19 / 20 / 20 / 13 / 3.2e-4 / 275
#     (3, 32, 128, 3)      0..19 / 20 /  7 / 15 / 1.3e-5 / 6.75      (1, (6, 5), 64, 4)   0..19 / 20 / 20 /  6 / 9.0e-4 / 389
#     (3, 32, 256, 2)      0..19 / 20 /  8 / 13 / 1.3e-5 / 6.28      (3, 32, 64, 5)       0..19 / 20 /  2 /  1 / 8.4e-6 / 3.16
#     (3, 32, 192, 2)      0..19 / 20 / 10 / 18 / 1.6e-5 / 7.47      (3, 32, 64, 33)      0..199 / 179 / 0: the best of the 200 is 0.96 (seed 153);
#                                                                                         kink-free and split only
# The one-sign-per-channel condition of 'kinkfree' and 'split' holds in fp64 for all eight cases with KINK_FREE_SEED; the smallest
# |pre-activation| is 0.68, at (3, 32, 64, 33) kink-free.  The whole model: 17 norms, one sign per channel, 0.85 / 1.62.
SEEDS = {(1, 28, 64, 2): 5, (3, 32, 128, 3): 15, (3, 32, 256, 2): 13, (3, 32, 192, 2): 18, (3, (12, 9), 64, 2): 13, (1, (6, 5), 64, 4): 6,
         (3, 32, 64, 5): 1}


def shape_of(case):
    """(N, in_ch, H, W)"""
    cin, side, _, n = case
    h, w = side if isinstance(side, tuple) else (side, side)
    return n, cin, h, w


def stem_pair(case, seed, mode='ordinary'):
    """(the fp32 `norm='batch'` residual stem of a case, its fp64 copy)"""
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    stem = nof.ODENet(case[0], out=10, n_filters=case[2], downsample='residual', adjoint=True, norm='batch').downsample.module
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in stem.named_parameters():
            if 'norm' in name:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if name.endswith('.bias'):
                    if mode == 'kinkfree':
                        p.add_(8.0)
                    elif mode == 'split':
                        p[0::2] += 8.0
                        p[1::2] -= 8.0
    return stem, copy.deepcopy(stem).double()


def case_inputs(case, seed):
    """(x, cotangent) of a case"""
    gen = torch.Generator().manual_seed(seed + 2)
    n, cin, h, w = shape_of(case)
    x = torch.randn(n, cin, h, w, generator=gen)
    o = lambda s: ((s - 2 - 1) // 2 + 1 - 1) // 2 + 1
    return x, torch.randn(n, case[2], o(h), o(w), generator=gen)


def norms_of(stem):
    return [stem[1].norm1, stem[1].norm2, stem[2].norm1, stem[2].norm2]


def preactivations(stem, x):
    """the outputs of the four norms of a CPU run of the module sequence"""
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())) for m in norms_of(stem)]
    with torch.no_grad():
        torch.nn.Sequential.forward(stem, x)
    for h in hooks:
        h.remove()
    return outs


@functools.lru_cache(maxsize=None)
def margin_ratio(case, seed):
    """Ordinary parameters: (every ReLU mask of the fp32 and the fp64 CPU run agrees, margin = the smallest |pre-activation| of
    the fp64 run, margin / the largest |fp32 pre-activation - fp64 pre-activation|)"""
    stem, ref = stem_pair(case, seed)
    x, _ = case_inputs(case, seed)
    p32, p64 = preactivations(stem, x), preactivations(ref, x.double())
    assert len(p64) == 4
    agree = all(torch.equal(a > 0, b > 0) for a, b in zip(p32, p64))
    margin = min(float(b.abs().min()) for b in p64)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    return agree, margin, margin / err


def sign_condition(case, mode):
    """The fp64 CPU run of a 'kinkfree' or 'split' set: (every channel of every norm's output has one sign over all rows, the
    smallest |pre-activation|)"""
    _, ref = stem_pair(case, KINK_FREE_SEED, mode)
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


def run_stem(stem, x, cot, forward=None):
    """Forward + backward: (out, d_x, parameter gradients by name, ()).  `forward`: how to call the stem (default: the module
    sequence, nn.Sequential.forward)."""
    xg = x.clone().requires_grad_(True)
    for p in stem.parameters():
        p.grad = None
    out = (forward or (lambda m, v: torch.nn.Sequential.forward(m, v)))(stem, xg)
    out.backward(cot)
    return out.detach(), xg.grad, {k: p.grad.clone() for k, p in stem.named_parameters()}, ()


@functools.lru_cache(maxsize=None)
def references(case, mode):
    """Computed once and shared, never modified: (the fp64 CPU run, the fp32 CPU run of the module operations), each as `run_stem`
    returns it.  The fp32 run is what the second term of the bounds is taken from."""
    seed = seed_of(case, mode)
    stem, ref = stem_pair(case, seed, mode)
    x, cot = case_inputs(case, seed)
    return run_stem(ref, x.double(), cot.double()), run_stem(stem, x, cot)


def bound(cpu_err):
    """per quantity: tests/test_gpu_stem.py's 2e-5, or 4 x the error of the fp32 modules on the CPU where that is larger
    (tests/test_gpu_bnfunc.py's allowance for two correct fp32 summation orders)"""
    return max(2e-5, 4 * cpu_err)


# ---------------------------------------------------------------------------------------------------------------------
# The whole model: ResNet(3, n_filters=64, downsample='residual', norm='batch') at [4, 3, 32, 32] -- this stem, six blocks at 8 x 8,
# the BatchNorm head: eight residual blocks.  Kink-free and split only, with KINK_FREE_SEED, as tests/bntrunk_cases.py runs its model.
# ---------------------------------------------------------------------------------------------------------------------
MODEL_SHAPE = (4, 3, 32, 32)
MODEL_MODES = ('kinkfree', 'split')
MODEL_BLOCKS = 8


def model_pair(seed, mode):
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    net = nof.ResNet(3, n_filters=64, downsample='residual', norm='batch')
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if 'norm' in name or name.startswith('classifier.module.0.'):
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
    """the fp64 CPU run of the whole model: (one sign per channel of every BatchNorm output, the smallest |pre-activation|)"""
    _, ref = model_pair(KINK_FREE_SEED, mode)
    x, _ = model_inputs(KINK_FREE_SEED)
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())) for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d)]
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

"""Cases, parameters and fp64 references of tests/test_gpu_bnhead.py: the `norm='batch'` classifier head up to its Linear layer,
BatchNorm2d(C, track_running_stats=False) -> ReLU -> AdaptiveAvgPool2d((1, 1)) -> dropout scale (model.py:231-250 with
model.py:274), as two HIP launches each way (head.py `bn_head_pool`, csrc/kernels_bnhead.hip).

The reference is that module sequence as `.double()` on the CPU.  Parameter sets as in tests/bnfunc_cases.py: the norm's weight
and bias perturbed by 0.2 randn ('ordinary'), the bias at +8 ('kinkfree') or +8 / -8 by channel parity ('split').  Seeds of the
ordinary runs by that file's recipe (`python tests/bnhead_cases.py`): the ReLU mask of the fp32 and the fp64 CPU run agree and the
margin ratio is at least bnfunc_cases.RATIO_YARDSTICK's; of seeds 0..19 the admissible one with the largest margin."""
import functools
import os
import sys

import torch
from torch import nn

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bnfunc_cases as B  # noqa: E402

MODES = B.MODES
KINK_FREE_SEED = B.KINK_FREE_SEED
# (N, C, H, W)
CASES = [(2, 64, 8, 8), (3, 64, 7, 7), (1, 64, 6, 5), (2, 192, 8, 8), (2, 256, 8, 8),
         (84, 64, 7, 7)]        # 21 chunks of four samples: many statistic partials
OFFSET_CASE = (4, 64, 8, 8)     # x = 50 + randn: the variance must survive a mean much larger than the spread
OFFSET = 50.0
# the table `python tests/bnhead_cases.py` printed: admissible of seeds 0..19 / kept / smallest |pre-activation| / margin over error
#     (2, 64, 8, 8)   20 /  2 / 4.3e-4 / 1148       (2, 256, 8, 8)   20 /  5 / 1.7e-4 / 375
#     (3, 64, 7, 7)   20 / 17 / 6.1e-4 / 1046       (84, 64, 7, 7)   10 / 11 / 1.2e-5 / 20.0
#     (1, 64, 6, 5)   20 / 11 / 2.1e-3 / 5348       (4, 64, 8, 8) at x = 50 + randn   17 / 16 / 2.6e-4 / 63.8
#     (2, 192, 8, 8)  20 / 19 / 2.1e-4 / 309
SEEDS = {(2, 64, 8, 8): 2, (3, 64, 7, 7): 17, (1, 64, 6, 5): 11, (2, 192, 8, 8): 19, (2, 256, 8, 8): 5, (84, 64, 7, 7): 11,
         (4, 64, 8, 8): 16}


def offset_of(case):
    return OFFSET if case == OFFSET_CASE else 0.0


def norm_pair(case, seed, mode='ordinary'):
    torch.manual_seed(seed)
    bn = nn.BatchNorm2d(case[1], track_running_stats=False)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in bn.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=gen))
        if mode == 'kinkfree':
            bn.bias.add_(8.0)
        elif mode == 'split':
            bn.bias[0::2] += 8.0
            bn.bias[1::2] -= 8.0
    ref = nn.BatchNorm2d(case[1], track_running_stats=False).double()
    ref.load_state_dict({k: v.double() for k, v in bn.state_dict().items()})
    return bn, ref


def case_inputs(case, seed):
    """(z, cotangent [N, C], dropout scale [N, C] of p = 0.5)"""
    gen = torch.Generator().manual_seed(seed + 2)
    n, c = case[:2]
    z = torch.randn(*case, generator=gen) + offset_of(case)
    cot = torch.randn(n, c, generator=gen)
    scale = (torch.rand(n, c, generator=gen) < 0.5).float() * 2.0
    return z, cot, scale


@functools.lru_cache(maxsize=None)
def margin_ratio(case, seed):
    bn, ref = norm_pair(case, seed)
    z = case_inputs(case, seed)[0]
    with torch.no_grad():
        p32, p64 = bn(z), ref(z.double())
    margin = float(p64.abs().min())
    return torch.equal(p32 > 0, p64 > 0), margin, margin / float((p32.double() - p64).abs().max())


def run_modules(bn, z, cot, scale):
    """(pooled, dz, dgamma, dbeta) of the module sequence"""
    zg = z.clone().requires_grad_(True)
    for p in bn.parameters():
        p.grad = None
    pooled = nn.functional.adaptive_avg_pool2d(torch.relu(bn(zg)), (1, 1)).flatten(1)
    if scale is not None:
        pooled = pooled * scale
    pooled.backward(cot)
    return pooled.detach(), zg.grad, bn.weight.grad.clone(), bn.bias.grad.clone()


def seed_of(case, mode):
    return SEEDS[case] if mode == 'ordinary' else KINK_FREE_SEED


@functools.lru_cache(maxsize=None)
def references(case, mode, dropout):
    """(the fp64 CPU run, the fp32 CPU run, S), computed once and shared.  S = max |gamma| / sigma x max |dy|: the size of dz without
    the cancellation inside BatchNorm's backward (`errors` says what for)."""
    seed = seed_of(case, mode)
    bn, ref = norm_pair(case, seed, mode)
    z, cot, scale = case_inputs(case, seed)
    scale = scale if dropout else None
    sigma = (z.double().var(dim=(0, 2, 3), unbiased=False) + ref.eps).sqrt()
    dy = (cot if scale is None else cot * scale).double().abs().max() / (case[2] * case[3])
    S = float((ref.weight.detach().abs() / sigma).max() * dy)
    return (run_modules(ref, z.double(), cot.double(), None if scale is None else scale.double()), run_modules(bn, z, cot, scale), S)


NAMES = ('pooled', 'dz', 'dgamma', 'dbeta')
FLOORS = {'pooled': 1e-5, 'dz': 2e-5, 'dgamma': 2e-5, 'dbeta': 2e-5}      # tests/test_gpu_head.py's bounds for the GroupNorm head


def errors(got, r64, S):
    """max-norm error over max|ref|; dz relative to max(max|ref|, 1e-4 S), as the project takes gradients that may vanish
    identically (tests/test_gpu_generic.py::_grads_close): with ONE sample and every pixel of a channel on the same side of the ReLU --
    (1, 64, 6, 5) kink-free and split -- dy is constant over the channel, dz and dgamma are zero identically and their max|ref| is
    rounding noise.  dgamma and dbeta likewise relative to max(max|ref|, 1e-4 x the larger of the two)."""
    def rel(a, b, floor=0.0):
        return float((a.detach().cpu().double() - b).abs().max() / max(float(b.abs().max()), floor))
    gmax = max(float(r64[2].abs().max()), float(r64[3].abs().max()))
    return {'pooled': rel(got[0], r64[0]), 'dz': rel(got[1], r64[1], 1e-4 * S), 'dgamma': rel(got[2], r64[2], 1e-4 * gmax),
            'dbeta': rel(got[3], r64[3], 1e-4 * gmax)}


if __name__ == '__main__':
    need = B.margin_ratio(*B.RATIO_YARDSTICK)[2]
    for case in CASES + [OFFSET_CASE]:
        rows = [(s,) + margin_ratio(case, s) for s in range(20)]
        ok = [(m, s, r) for s, agree, m, r in rows if agree and r >= need]
        print(case, '%d admissible -> kept %s' % (len(ok), max(ok) if ok else None))

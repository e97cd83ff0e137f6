"""Cases, parameters and fp64 references shared by tests/test_bnfunc_host.py and tests/test_gpu_bnfunc.py: the `norm='batch'`
dynamics `ODEfunc(C, norm='batch')` (model.py:326-348 with model.py:274) as one HIP node (bnfunc.py, csrc/bnfunc_api.hip).

The reference of every comparison is the same `ODEfunc` as `.double()` on the CPU, called with an fp64 `t`: the module
operations, never the node.

Seeds of the ordinary-parameter runs (`SEEDS`) were chosen on the CPU as tests/test_gpu_resnet.py chooses its own: the
module operations run in fp32 and in fp64, and a seed is eligible only if EVERY ReLU mask (the sign of every output of
norm1 and norm2) agrees between the two; among the eligible seeds 0..19 of a case the one whose smallest |pre-activation| is
largest was kept (`python tests/bnfunc_cases.py` prints the table).  Every case has eligible seeds, so every case runs both ways
(BatchNorm pre-activations are O(1) and the dynamics are two layers deep: even the 524 288 pre-activations of (64, 64, 8, 8) keep
4.9e-6 clear of zero at seed 5).

`MULTI_CASES` are the launch regimes `CASES` does not reach, each with the properties of the plan it is there for, under three parameter
sets (ordinary with `MULTI_SEEDS`, kink-free, split); the comments next to them say how their seeds were admitted."""
import copy
import functools
import os
import sys

import torch

T_EVAL = 0.37
# (N, C, H, W)
CASES = [(2, 64, 8, 8),      # one row tile, one column tile
         (3, 64, 7, 7),      # 147 rows: ragged tile, odd batch
         (1, 64, 6, 5),      # one sample, non-square: catches H / W swaps in the time tables
         (2, 128, 8, 8),     # two column tiles
         (2, 192, 8, 8),     # three tiles, not a power of two
         (2, 256, 8, 8),     # the CIFAR width
         (1, 64, 16, 16),    # one-shot-stem states
         (64, 64, 8, 8)]     # 4096 rows: many statistic partials, split-K weight gradient
OFFSET_CASE = (4, 64, 8, 8)  # x = 50 + randn: the variance must survive a mean much larger than the spread
# chosen by the recipe of the docstring (`python tests/bnfunc_cases.py`)
SEEDS = {(2, 64, 8, 8): 2, (3, 64, 7, 7): 12, (1, 64, 6, 5): 17, (2, 128, 8, 8): 0, (2, 192, 8, 8): 6, (2, 256, 8, 8): 18,
         (1, 64, 16, 16): 11, (64, 64, 8, 8): 5}
KINK_FREE_SEED = 5

# ---------------------------------------------------------------------------------------------------------------------
# The launch regimes CASES does not reach.  Every BatchNorm pass walks its chunk as `for (r = r0 + rr; r < r1; r += 32)`, and every
# shape above (and every shape of tests/bnsolve_cases.py SHAPES / SPLITK_SHAPE) has chunks of 32 rows: one trip.  The CIFAR training
# step (128, 256, 8, 8) has chunks of 128 rows.  Each case below names the properties of the plan it is there for (REGIMES);
# tests/test_bnfunc_host.py asserts them through node_bnfunc_describe, so a later change of the chunk or split heuristics cannot
# quietly empty these cases.
# ---------------------------------------------------------------------------------------------------------------------
def reduce_lanes(ns):
    """k_bn_reduce sums ns slabs over four lanes, lane `sub` taking `for (k = sub; k + 4 < ns; k += 8) {two slabs}` and then
    `if (k < ns) {one slab}`: (the lanes that run the loop, the lanes that run the remainder line)."""
    loop, rest = set(), set()
    for sub in range(4):
        k = sub
        while k + 4 < ns:
            loop.add(sub)
            k += 8
        if k < ns:
            rest.add(sub)
    return loop, rest


REGIMES = {
    'two_trips': lambda d: d['chunk_rows'] > 32,
    'three_trips': lambda d: d['chunk_rows'] >= 96 and d['chunk_rows'] & (d['chunk_rows'] - 1) != 0,
    'short_last_chunk': lambda d: d['chunk_rows'] > 32 and 0 < d['last_chunk_rows'] < 32,        # half the row slots idle there
    'ragged_last_trip': lambda d: d['chunk_rows'] > 32 and d['last_chunk_rows'] % 32 != 0,
    'several_chunks': lambda d: d['nchunk'] > 4,                                                  # every chain of the four-way combination has > 1 link
    'nsplit_5_to_7': lambda d: 5 <= d['wgrad_nsplit'] <= 7,                                        # lane 0 in the loop, lanes 1-3 in the remainder
    'nsplit_8': lambda d: d['wgrad_nsplit'] == 8,
    'nsplit_loop_and_remainder': lambda d: all(len(s) == 4 for s in reduce_lanes(d['wgrad_nsplit'])),
    'nsplit_lanes_differ': lambda d: len(reduce_lanes(d['wgrad_nsplit'])[0]) not in (0, 4) or len(reduce_lanes(d['wgrad_nsplit'])[1]) not in (0, 4),
    'one_chunk': lambda d: d['nchunk'] == 1 and d['wgrad_nsplit'] == 1,
    'tiles_3': lambda d: d['column_tiles'] == 3,
    'tiles_4': lambda d: d['column_tiles'] == 4,
    'tiles_8': lambda d: d['column_tiles'] == 8,
    'tiles_16': lambda d: d['column_tiles'] == 16,
    # the cap on the number of chunks of a wide tensor (maxchunk 32 at C = 512, 16 at C = 1024) is what gives these rows two trips: at
    # C <= 256 (maxchunk >= 64) as many rows still run in chunks of 32
    'chunk_cap_of_wide_tensors': lambda d: d['chunk_rows'] > 32 and d['rows'] <= 64 * 32 and d['column_tiles'] >= 8,
}
# (N, C, H, W) -> the regimes it is there for
MULTI_CASES = {
    (5, 64, 8, 8): ('nsplit_5_to_7', 'nsplit_lanes_differ', 'several_chunks'),      # 320 rows
    (84, 64, 7, 7): ('two_trips', 'short_last_chunk', 'ragged_last_trip', 'nsplit_loop_and_remainder', 'several_chunks'),      # 4116 rows, 65 chunks, the last of 20 rows
    (33, 256, 8, 8): ('two_trips', 'tiles_4', 'several_chunks'),      # the CIFAR width
    (43, 192, 8, 8): ('two_trips', 'tiles_3', 'nsplit_8', 'several_chunks'),
    (2, 512, 4, 4): ('tiles_8', 'one_chunk'),      # the smallest tensor at eight column tiles
    (17, 512, 8, 8): ('two_trips', 'tiles_8', 'chunk_cap_of_wide_tensors', 'several_chunks'),
    (9, 1024, 8, 8): ('two_trips', 'tiles_16', 'chunk_cap_of_wide_tensors', 'several_chunks'),
    # 8232 rows: chunks of 96 rows (three trips, no power of two), the last of 72 = 32 + 32 + 8, 58 weight-gradient shares (two lanes of
    # k_bn_reduce end in the remainder line, two in the loop)
    (168, 64, 7, 7): ('three_trips', 'ragged_last_trip', 'nsplit_lanes_differ', 'several_chunks'),
}
# Parameter sets of the new cases: 'kinkfree' and 'split' with KINK_FREE_SEED, 'ordinary' with MULTI_SEEDS[case].
# An ordinary seed is admitted only if (a) every ReLU mask agrees between the fp32 and the fp64 CPU run, as for SEEDS, and (b) its
# margin ratio -- smallest |pre-activation| of the fp64 run over the largest error of an fp32 pre-activation (`margin_ratio`) -- is
# at least that of the closest case the suite already ran, RATIO_YARDSTICK.  The big cases sit much closer to a kink than the small
# ones, and a GPU summation order is a third fp32 rounding: without (b) a mask could differ for a reason other than a defect.
# Seeds 0..199 were searched once on the CPU (`python tests/bnfunc_cases.py multi`); among the admissible ones the seed with the
# largest margin was kept.  A case without an admissible seed has no entry and runs kink-free and split only.
RATIO_YARDSTICK = ((64, 64, 8, 8), 5)
# The search's table (the yardstick stands at 2.60): admissible seeds / kept / smallest |pre-activation| / margin over error
#     (5, 64, 8, 8)    179 / 103 / 2.3e-4 / 153       (2, 512, 4, 4)   183 / 24 / 1.8e-4 / 131
#     (84, 64, 7, 7)    17 /  32 / 8.7e-6 / 4.5       (17, 512, 8, 8)    1 / 65 / 8.2e-6 / 3.9
#     (33, 256, 8, 8)    3 / 168 / 5.8e-6 / 3.2       (9, 1024, 8, 8)    0: the best of the 200 is 2.06 (seed 177); kink-free and split only
#     (43, 192, 8, 8)    5 /  51 / 7.9e-6 / 4.8       (168, 64, 7, 7)    3 / 22 / 5.2e-6 / 3.2
MULTI_SEEDS = {(5, 64, 8, 8): 103, (84, 64, 7, 7): 32, (33, 256, 8, 8): 168, (43, 192, 8, 8): 51, (2, 512, 4, 4): 24, (17, 512, 8, 8): 65,
               (168, 64, 7, 7): 22}
MODES = ('ordinary', 'kinkfree', 'split')


def func_pair(C, seed, kink_free=False, mode=None):
    """(fp32 ODEfunc(C, norm='batch'), its fp64 copy): norm weights and biases perturbed by 0.2 randn.  mode (default: by
    `kink_free`): 'kinkfree': the biases of norm1 and norm2 (the norms in front of a ReLU) at +8, so that every pre-activation is
    positive and no mask can differ; 'split': +8 on the even channels and -8 on the odd ones, so that half the channels are masked
    on every row and half are live, with no pre-activation anywhere near zero."""
    import neural_ode_features_amd as nof
    mode = mode or ('kinkfree' if kink_free else 'ordinary')
    assert mode in MODES, mode
    torch.manual_seed(seed)
    func = nof.ODEfunc(C, norm='batch')
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in func.named_parameters():
            if 'norm' in name:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if name in ('norm1.bias', 'norm2.bias'):
                    if mode == 'kinkfree':
                        p.add_(8.0)
                    elif mode == 'split':
                        p[0::2] += 8.0
                        p[1::2] -= 8.0
    return func, copy.deepcopy(func).double()


def case_inputs(case, seed, offset=0.0):
    """(x, cotangent) of a case"""
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(*case, generator=gen)
    return x + offset, torch.randn(*case, generator=gen)


def relu_masks(func, x, t):
    """(the sign of every output of norm1 and norm2 of a CPU run, the smallest |pre-activation|)"""
    masks, margin = [], [float('inf')]

    def hook(m, i, o):
        masks.append(o > 0)
        margin[0] = min(margin[0], float(o.abs().min()))
    hooks = [func.norm1.register_forward_hook(hook), func.norm2.register_forward_hook(hook)]
    with torch.no_grad():
        func(t, x)
    for h in hooks:
        h.remove()
    return masks, margin[0]


def masks_agree(case, seed):
    """(every ReLU mask of the fp32 and the fp64 CPU run agrees, smallest |pre-activation| of the fp64 run)"""
    func, ref = func_pair(case[1], seed)
    x, _ = case_inputs(case, seed)
    m32, _ = relu_masks(func, x, torch.tensor(T_EVAL))
    m64, margin = relu_masks(ref, x.double(), torch.tensor(T_EVAL, dtype=torch.float64))
    return all(torch.equal(a, b) for a, b in zip(m32, m64)), margin


def preactivations(func, x, t):
    """the outputs of norm1 and norm2 of a CPU run"""
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach())) for m in (func.norm1, func.norm2)]
    with torch.no_grad():
        func(t, x)
    for h in hooks:
        h.remove()
    return outs


@functools.lru_cache(maxsize=None)
def margin_ratio(case, seed):
    """Ordinary parameters: (every ReLU mask of the fp32 and the fp64 CPU run agrees, margin = the smallest |pre-activation| of the
    fp64 run, margin / the largest |fp32 pre-activation - fp64 pre-activation|)"""
    func, ref = func_pair(case[1], seed)
    x, _ = case_inputs(case, seed)
    p32 = preactivations(func, x, torch.tensor(T_EVAL))
    p64 = preactivations(ref, x.double(), torch.tensor(T_EVAL, dtype=torch.float64))
    agree = all(torch.equal(a > 0, b > 0) for a, b in zip(p32, p64))
    margin = min(float(b.abs().min()) for b in p64)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    return agree, margin, margin / err


def sign_condition(case, seed, mode):
    """The fp64 CPU run of a 'kinkfree' or 'split' parameter set: (every channel of norm1's and norm2's output has one sign over all
    rows, the fraction of positive channels per norm, the smallest |pre-activation|)"""
    _, ref = func_pair(case[1], seed, mode=mode)
    x, _ = case_inputs(case, seed)
    constant, on, margin = True, [], float('inf')
    for o in preactivations(ref, x.double(), torch.tensor(T_EVAL, dtype=torch.float64)):
        pos = (o > 0).permute(1, 0, 2, 3).reshape(o.shape[1], -1)
        constant = constant and bool((pos.all(dim=1) | (~pos).all(dim=1)).all())
        on.append(float(pos.all(dim=1).double().mean()))
        margin = min(margin, float(o.abs().min()))
    return constant, on, margin


def _run_modules(func, x, cot, t):
    """Forward + backward of the module operations on the CPU: (out, d_x, d_t, parameter gradients by name, S) with S[name] =
    sum over (n, y, x) of |dL/d(convolution output)| per channel for the two convolutions (a tensor hook on their outputs)."""
    xg = x.clone().requires_grad_(True)
    tg = t.clone().requires_grad_(True)
    S, hooks = {}, []

    def watch(name):
        def fwd_hook(m, i, o):
            o.register_hook(lambda g: S.__setitem__(name, g.detach().abs().sum(dim=(0, 2, 3))))
        return fwd_hook
    for name in ('conv1', 'conv2'):
        hooks.append(getattr(func, name)._layer.register_forward_hook(watch(name)))
    for p in func.parameters():
        p.grad = None
    out = func(tg, xg)
    out.backward(cot)
    for h in hooks:
        h.remove()
    return out.detach(), xg.grad, tg.grad, {k: p.grad.clone() for k, p in func.named_parameters()}, S


@functools.lru_cache(maxsize=None)
def references(case, seed, kink_free, t=T_EVAL, offset=0.0, mode=None):
    """Computed once and shared, never modified: (the fp64 CPU run, the fp32 CPU run of the module operations), each as
    `_run_modules` returns it.  The fp32 run is what the bounds are taken from (4 x its own error against fp64)."""
    func, ref = func_pair(case[1], seed, kink_free, mode)
    x, cot = case_inputs(case, seed, offset)
    r64 = _run_modules(ref, x.double(), cot.double(), torch.tensor(t, dtype=torch.float64))
    r32 = _run_modules(func, x, cot, torch.tensor(t, dtype=torch.float32))
    return r64, r32


BIAS_NAMES = ('conv1._layer.bias', 'conv2._layer.bias')


def errors(got, r64):
    """max-norm error over max|ref| of (out, d_x, d_t, grads) against the fp64 run: output, d_x and d_t relative to their own
    scale, parameter gradients relative to max(max|ref|, 1e-4 x the largest gradient) as tests/test_gpu_generic.py::_grads_close
    does.  The two convolution biases are left out (their gradient is zero identically: `bias_ratio`)."""
    out, dx, dt, grads = got
    out_r, dx_r, dt_r, grads_r, _ = r64

    def rel(a, b, scale=None):
        a, b = a.detach().cpu().double().reshape(-1), b.reshape(-1)
        return float((a - b).abs().max() / (b.abs().max() if scale is None else scale))
    errs = {'output': rel(out, out_r), 'd_x': rel(dx, dx_r), 'd_t': rel(dt, dt_r)}
    gmax = max(float(g.abs().max()) for k, g in grads_r.items() if k not in BIAS_NAMES)
    for k, g in grads_r.items():
        if k not in BIAS_NAMES:
            errs['grad ' + k] = rel(grads[k], g, max(float(g.abs().max()), 1e-4 * gmax))
    return errs


def bias_ratio(grads, r64):
    """max over the channels of |d bias[c]| / S[c] for both convolutions, S from the fp64 run (channels with S[c] == 0 -- conv1's
    behind a mask that is off on every row, in the 'split' sets -- are left to `bias_within`)"""
    S = r64[4]
    worst = 0.0
    for k in BIAS_NAMES:
        g, s = grads[k].detach().cpu().double().abs(), S[k.split('.')[0]]
        live = s > 0
        if live.any():
            worst = max(worst, float((g[live] / s[live]).max()))
    return worst


def bias_within(grads, r64, factor):
    """|d bias[c]| <= factor x S[c] for every channel of both convolutions (no division: S[c] == 0 demands an exact zero)"""
    S = r64[4]
    return all(bool((grads[k].detach().cpu().double().abs() <= factor * S[k.split('.')[0]]).all()) for k in BIAS_NAMES)


if __name__ == '__main__':      # the seed tables of the docstring and of MULTI_SEEDS (CPU only)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ['multi']:
        need = margin_ratio(*RATIO_YARDSTICK)[2]
        print('yardstick %s seed %d: margin / error %.2f' % (RATIO_YARDSTICK + (need,)))
        for case in MULTI_CASES:
            rows = [(s,) + margin_ratio(case, s) for s in range(200)]
            ok = [(m, s, r) for s, agree, m, r in rows if agree and r >= need]
            best = max(rows, key=lambda r: r[3])
            if ok:
                print(case, '%d admissible seeds -> kept %d, smallest |pre-activation| %.2e, margin / error %.2f' % (len(ok), max(ok)[1], max(ok)[0], max(ok)[2]))
            else:
                print(case, 'no admissible seed (best margin / error %.2f at seed %d): kink-free and split only' % (best[3], best[0]))
        sys.exit(0)
    for case in CASES:
        rows = [(s,) + masks_agree(case, s) for s in range(20)]
        ok = [(m, s) for s, agree, m in rows if agree]
        if ok:
            print(case, 'eligible seeds:', [s for _, s in ok], '-> kept', max(ok)[1], 'smallest |pre-activation| %.2e' % max(ok)[0])
        else:
            print(case, 'no eligible seed: kink-free only')

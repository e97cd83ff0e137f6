"""Cases, parameters and fp64 references shared by tests/test_bntrunk_host.py and tests/test_gpu_bntrunk.py: the `norm='batch'`
residual trunk, `blocks` x ResBlock(C, C, norm='batch') (model.py:79, :284-310 with model.py:274), as one HIP node (resnet.py
`_BnTrunkFn`, csrc/bntrunk_api.hip).

The reference of every comparison is the same `ResidualTrunk` as `.double()` on the CPU, run block by block: the module
operations, never the node.

Parameter sets are those of tests/bnfunc_cases.py::func_pair: norm weights and biases perturbed by 0.2 randn ('ordinary'), and +8
('kinkfree') or +8 / -8 by channel parity ('split') on the biases of the norms in front of a ReLU -- here every norm of the trunk.

Seeds of the ordinary runs follow that file's recipe (`python tests/bntrunk_cases.py` prints the table): the module operations
run in fp32 and in fp64 on the CPU, and a seed is admitted only if (a) EVERY ReLU mask (the sign of every output of norm1 and norm2
of every block) agrees between the two and (b) its margin ratio -- smallest |pre-activation| of the fp64 run over the largest
error of an fp32 pre-activation -- is at least bnfunc_cases.RATIO_YARDSTICK's (2.60): a GPU summation order is a third fp32
rounding, and without (b) a mask could differ for a reason other than a defect.  (b) is asked of EVERY case here, not only of
the multi-row ones: the trunk is up to twelve layers deep and (256, 8, 2, 6) sits at 2.55 at the best of seeds 0..19.  Seeds 0..19
are searched first, 0..199 if none of them is admissible; among the admissible seeds the one with the largest margin is kept.  A
case without an entry in SEEDS has no admissible seed and runs kink-free and split only."""
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
# (C, side, N, blocks); side: H = W, or (H, W)
CASES = [(64, 8, 2, 1),         # one block, one column tile
         (64, 7, 3, 2),         # 147 rows: ragged tile, odd batch
         (128, 8, 2, 6),        # full depth
         (256, 8, 2, 6),        # the CIFAR width
         (192, 8, 2, 2),        # three column tiles, not a power of two: the GroupNorm trunk refuses it
         (64, 16, 1, 2),        # one-shot-stem states
         (64, (6, 5), 1, 1),    # one sample, H != W
         (64, 1, 4, 1)]         # 1 x 1 images: below the dynamics' h, w >= 3 (no time channel here, so no border classes)
# the launch regimes of bnfunc_cases.MULTI_CASES that carry over (the chunks come from the same bn_chunk_rows), two blocks each
MULTI_CASES = {
    (64, 7, 84, 2): ('two_trips', 'short_last_chunk', 'ragged_last_trip', 'several_chunks'),
    (256, 8, 33, 2): ('two_trips', 'tiles_4', 'several_chunks'),
    (64, 8, 5, 2): ('nsplit_5_to_7', 'several_chunks'),
}
ALL_CASES = CASES + list(MULTI_CASES)
# chosen by the recipe of the docstring (`python tests/bntrunk_cases.py`); the table it printed (the yardstick stands at 2.60):
# seeds searched / with equal masks / admissible / kept / smallest |pre-activation| / margin over error
#     (64, 8, 2, 1)      0..19 / 20 / 19 /  5 / 1.6e-4 / 137       (64, (6, 5), 1, 1)  0..19 / 20 / 20 /  4 / 1.0e-3 / 961
#     (64, 7, 3, 2)      0..19 / 20 / 18 /  8 / 1.3e-4 / 83        (64, 1, 4, 1)       0..19 / 20 / 20 / 10 / 6.0e-3 / 5357
#     (128, 8, 2, 6)     0..19 / 20 / 10 / 15 / 2.8e-5 / 14.7      (64, 7, 84, 2)      0..19 / 20 /  1 /  5 / 6.9e-6 / 3.77
#     (256, 8, 2, 6)     0..19 / 20 /  1 /  9 / 5.7e-6 / 2.78      (64, 8, 5, 2)       0..19 / 20 / 15 /  3 / 5.3e-5 / 39.1
#     (192, 8, 2, 2)     0..19 / 20 / 18 /  3 / 3.5e-5 / 24.6      (256, 8, 33, 2)     0..199 / 186 / 0: the best of the 200 is 1.31 (seed 52);
#     (64, 16, 1, 2)     0..19 / 20 / 12 /  9 / 8.2e-5 / 40.5                          kink-free and split only
SEEDS = {(64, 8, 2, 1): 5, (64, 7, 3, 2): 8, (128, 8, 2, 6): 15, (256, 8, 2, 6): 9, (192, 8, 2, 2): 3, (64, 16, 1, 2): 9,
         (64, (6, 5), 1, 1): 4, (64, 1, 4, 1): 10, (64, 7, 84, 2): 5, (64, 8, 5, 2): 3}


def shape_of(case):
    """(N, C, H, W)"""
    c, side, n, _ = case
    h, w = side if isinstance(side, tuple) else (side, side)
    return n, c, h, w


def trunk_pair(case, seed, mode='ordinary'):
    """(fp32 ResidualTrunk(C, blocks, norm='batch'), its fp64 copy), parameters as bnfunc_cases.func_pair sets them"""
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    trunk = nof.resnet.ResidualTrunk(case[0], case[3], norm='batch')
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in trunk.named_parameters():
            if 'norm' in name:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
                if name.endswith('.bias'):
                    if mode == 'kinkfree':
                        p.add_(8.0)
                    elif mode == 'split':
                        p[0::2] += 8.0
                        p[1::2] -= 8.0
    return trunk, copy.deepcopy(trunk).double()


def case_inputs(case, seed, offset=0.0):
    """(x, cotangent) of a case"""
    gen = torch.Generator().manual_seed(seed + 2)
    shape = shape_of(case)
    x = torch.randn(*shape, generator=gen)
    return x + offset, torch.randn(*shape, generator=gen)


def preactivations(trunk, x):
    """the outputs of norm1 and norm2 of every block of a CPU run"""
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach())) for blk in trunk for m in (blk.norm1, blk.norm2)]
    with torch.no_grad():
        torch.nn.Sequential.forward(trunk, x)
    for h in hooks:
        h.remove()
    return outs


@functools.lru_cache(maxsize=None)
def margin_ratio(case, seed):
    """Ordinary parameters: (every ReLU mask of the fp32 and the fp64 CPU run agrees, margin = the smallest |pre-activation| of
    the fp64 run, margin / the largest |fp32 pre-activation - fp64 pre-activation|)"""
    trunk, ref = trunk_pair(case, seed)
    x, _ = case_inputs(case, seed)
    p32, p64 = preactivations(trunk, x), preactivations(ref, x.double())
    agree = all(torch.equal(a > 0, b > 0) for a, b in zip(p32, p64))
    margin = min(float(b.abs().min()) for b in p64)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    return agree, margin, margin / err


def sign_condition(case, mode):
    """The fp64 CPU run of a 'kinkfree' or 'split' set: (every channel of every norm's output has one sign over all rows, the
    smallest |pre-activation|)"""
    _, ref = trunk_pair(case, KINK_FREE_SEED, mode)
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


def run_modules(trunk, x, cot):
    """Forward + backward of the module operations, block by block: (out, d_x, parameter gradients by name, taps)"""
    xg = x.clone().requires_grad_(True)
    for p in trunk.parameters():
        p.grad = None
    h, taps = xg, []
    for blk in trunk:
        h = blk(h)
        taps.append(h.detach())
    h.backward(cot)
    return h.detach(), xg.grad, {k: p.grad.clone() for k, p in trunk.named_parameters()}, taps


@functools.lru_cache(maxsize=None)
def references(case, mode):
    """Computed once and shared, never modified: (the fp64 CPU run, the fp32 CPU run of the module operations), each as
    `run_modules` returns it.  The fp32 run is what the second term of the bounds is taken from."""
    seed = seed_of(case, mode)
    trunk, ref = trunk_pair(case, seed, mode)
    x, cot = case_inputs(case, seed)
    return run_modules(ref, x.double(), cot.double()), run_modules(trunk, x, cot)


def errors(got, r64):
    """max-norm error over max|ref| of (out, d_x, grads, taps) against the fp64 run; parameter gradients relative to
    max(max|ref|, 1e-4 x the largest gradient)"""
    out, dx, grads, taps = got
    out_r, dx_r, grads_r, taps_r = r64

    def rel(a, b, scale=None):
        a, b = a.detach().cpu().double().reshape(-1), b.reshape(-1)
        return float((a - b).abs().max() / (b.abs().max() if scale is None else scale))
    errs = {'output': rel(out, out_r), 'd_x': rel(dx, dx_r)}
    for i, (a, b) in enumerate(zip(taps, taps_r)):
        errs['tap %d' % i] = rel(a, b)
    gmax = max(float(g.abs().max()) for g in grads_r.values())
    for k, g in grads_r.items():
        errs['grad ' + k] = rel(grads[k], g, max(float(g.abs().max()), 1e-4 * gmax))
    return errs


def bound(blocks, cpu_err):
    """per quantity: tests/test_gpu_resnet.py::bound, or 4 x the error of the fp32 modules on the CPU where that is larger
    (tests/test_gpu_bnfunc.py's allowance for two correct fp32 summation orders)"""
    return max(2e-5 * max(1.0, blocks / 2), 4 * cpu_err)


# ---------------------------------------------------------------------------------------------------------------------
# The whole model: ResNet(3, n_filters=64, downsample='one-shot', norm='batch') at [4, 3, 32, 32] -- a 4x4 / 2 convolution, six
# blocks at 16 x 16, the BatchNorm head.  The recipe above over its thirteen norms in front of a ReLU (851 968 pre-activations;
# `python tests/bntrunk_cases.py model`) admits NO seed for ordinary parameters: of seeds 0..199, 184 keep every mask between fp32
# and fp64, and the best margin / error among them is 1.88 (seed 128) against the yardstick's 2.60.  So the model runs kink-free and
# split only (MODEL_MODES), with KINK_FREE_SEED, as a case without an admissible seed does.
# ---------------------------------------------------------------------------------------------------------------------
MODEL_SHAPE = (4, 3, 32, 32)
MODEL_MODES = ('kinkfree', 'split')


def model_pair(seed, mode='ordinary'):
    import neural_ode_features_amd as nof
    assert mode in MODES, mode
    torch.manual_seed(seed)
    net = nof.ResNet(3, n_filters=64, downsample='one-shot', norm='batch')
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


def _model_preactivations(net, x):
    outs = []
    # (a copy: the head's ReLU works in place)
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone())) for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return outs


@functools.lru_cache(maxsize=None)
def model_margin_ratio(seed):
    net, ref = model_pair(seed)
    x, _ = model_inputs(seed)
    p32, p64 = _model_preactivations(net, x), _model_preactivations(ref, x.double())
    assert len(p64) == 13
    agree = all(torch.equal(a > 0, b > 0) for a, b in zip(p32, p64))
    margin = min(float(b.abs().min()) for b in p64)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))
    return agree, margin, margin / err


def run_model(net, x, cot):
    """(logits, d_x, parameter gradients by name) of a forward + backward"""
    xg = x.clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    out = net(xg)
    out.backward(cot)
    return out.detach(), xg.grad, {k: p.grad.clone() for k, p in net.named_parameters()}


@functools.lru_cache(maxsize=None)
def model_references(mode):
    """(the fp64 CPU run, the fp32 CPU run) of the whole model, each as `run_model` returns it, and the features [7, N, C] of both"""
    net, ref = model_pair(KINK_FREE_SEED, mode)
    x, cot = model_inputs(KINK_FREE_SEED)
    r64, r32 = run_model(ref, x.double(), cot.double()), run_model(net, x, cot)
    feats = []
    for m, xi in ((ref, x.double()), (net, x)):
        m = copy.deepcopy(m).eval()
        m.to_features_extractor()
        with torch.no_grad():
            feats.append(m(xi))
    return r64, r32, feats[0], feats[1]


def model_errors(got, r64):
    out, dx, grads = got
    out_r, dx_r, grads_r = r64

    def rel(a, b, scale=None):
        a, b = a.detach().cpu().double().reshape(-1), b.reshape(-1)
        return float((a - b).abs().max() / (b.abs().max() if scale is None else scale))
    errs = {'logits': rel(out, out_r), 'd_x': rel(dx, dx_r)}
    gmax = max(float(g.abs().max()) for g in grads_r.values())
    for k, g in grads_r.items():
        errs['grad ' + k] = rel(grads[k], g, max(float(g.abs().max()), 1e-4 * gmax))
    return errs


if __name__ == '__main__':      # the seed table (CPU only)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    need = B.margin_ratio(*B.RATIO_YARDSTICK)[2]
    print('yardstick %s seed %d: margin / error %.2f' % (B.RATIO_YARDSTICK + (need,)))
    if sys.argv[1:] == ['model']:
        rows = [(s,) + model_margin_ratio(s) for s in range(20)]
        ok = [(m, s, r) for s, agree, m, r in rows if agree and r >= need]
        if not ok:
            rows = [(s,) + model_margin_ratio(s) for s in range(200)]
            ok = [(m, s, r) for s, agree, m, r in rows if agree and r >= need]
        print('whole model, seeds 0..%d: %d with equal masks, %d admissible -> kept %s; best margin / error %.2f at seed %d'
              % (len(rows) - 1, sum(1 for r in rows if r[1]), len(ok), max(ok) if ok else None, max(rows, key=lambda r: r[3])[3], max(rows, key=lambda r: r[3])[0]))
        sys.exit(0)
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

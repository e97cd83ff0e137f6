#!/usr/bin/env python
"""Times of the `convolution` stem (convstem.py) and of the `ode2` stem's hand-off (downconv.py) against the module sequences
they replace -- `nn.Sequential.forward` / `ODEDownsample2.fused_handoff = False` (MIOpen / ATen plus the fused GroupNorm + ReLU
node) -- in ONE process, alternating the two:

    python3 tools/convstem_time.py > profiles/convstem_time.txt

Per shape: forward (inference, under no_grad) and forward + backward (torch.autograd.grad of every parameter; the hand-off also
of its input, which the solve in front of it needs), each as HIP events around a window of `--reps` calls from Python (what a
training step sees: dispatch included), alternating the two paths round by round, median over the rounds.  The operands of a
call -- the input and the output gradient -- ROTATE through enough buffers to exceed the 256 MB Infinity Cache between two uses
of one of them, so they arrive cache-cold; activations live in the workspace (fused) or come from the caching allocator
(modules), the same blocks call after call, for both paths alike.  Next to the times: the device kernels one forward + backward
launches on either path (torch.profiler), and the worst error of the fused results against the fp64 modules, in max norm and in
relative L2 (at batch 128 a few of the stem's 9 M pre-activations land within fp32 rounding of zero and their ReLU masks differ
from the fp64 run's, which moves single gradient entries by ~1 % on either path: tests/test_gpu_convstem.py pins the numerics)."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--n', type=int, default=128)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from torch import nn
    import neural_ode_features_amd as nof
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s; %d calls per timed window, median of %d rounds, paths alternating' % (torch.cuda.get_device_name(0), a.reps, a.rounds))

    def window(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()

        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.reps
        return run

    def kernels(fn):
        """device kernels of one call, or None where the profiler cannot see the device"""
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                    and 'memset' not in e.name.lower())
            return n or None
        except Exception as exc:       # noqa: BLE001
            print('(no kernel count: %s)' % exc)
            return None

    def measure(title, paths, xs, cots, wrt_of, ref_err):
        """paths: name -> forward callable; wrt_of: name -> tensors whose gradient the backward produces"""
        i = [0]

        def nxt():
            i[0] = (i[0] + 1) % len(xs)
            return xs[i[0]], cots[i[0]]

        def fwd(name):
            def fn():
                with torch.no_grad():
                    paths[name](nxt()[0])
            return fn

        def both(name):
            def fn():
                x, c = nxt()
                torch.autograd.grad(paths[name](x), wrt_of(name, x), c)
            return fn
        print('\n%s' % title)
        print('operands rotate through %d buffers (%.0f MB); fused against the fp64 modules: worst max error / max|ref| %.2e, worst relative L2 %.2e'
              % ((len(xs), len(xs) * (xs[0].numel() + cots[0].numel()) * 4 / 1e6) + ref_err))
        print('%-20s %12s %12s %10s' % ('', 'fused us', 'modules us', 'ratio'))
        for what, make in (('forward', fwd), ('forward + backward', both)):
            runs = {p: window(make(p)) for p in paths}
            t = {p: [] for p in runs}
            for _ in range(a.rounds):
                for p in runs:
                    t[p].append(runs[p]())
            med = {p: statistics.median(v) for p, v in t.items()}
            print('%-20s %12.1f %12.1f %10.2f     (min %.1f / %.1f, max %.1f / %.1f)'
                  % (what, med['fused'], med['modules'], med['modules'] / med['fused'], min(t['fused']), min(t['modules']),
                     max(t['fused']), max(t['modules'])))
        counts = {p: kernels(both(p)) for p in paths}
        print('device kernels per forward + backward: fused %s, modules %s' % (counts['fused'], counts['modules']))

    def buffers(shape_x, shape_c, requires_grad):
        per = 4 * (torch.Size(shape_x).numel() + torch.Size(shape_c).numel())
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // per)))
        xs = [torch.randn(shape_x, device='cuda').requires_grad_(requires_grad) for _ in range(nsets)]
        return xs, [torch.randn(shape_c, device='cuda') for _ in range(nsets)]

    def worst(got, ref):
        pairs = [(g.detach().double().cpu(), r.detach()) for g, r in zip(got, ref)]
        return (max(float((g - r).abs().max() / r.abs().max()) for g, r in pairs), max(float((g - r).norm() / r.norm()) for g, r in pairs))

    # ---- the `convolution` stem ------------------------------------------------------------------------------------
    torch.manual_seed(0)
    stem = nof.ODENet(3, n_filters=256, downsample='convolution').downsample.module
    ref = copy.deepcopy(stem).double()
    stem = stem.cuda()
    params = list(stem.parameters())
    xs, cots = buffers((a.n, 3, 32, 32), (a.n, 256, 7, 7), False)
    out = stem(xs[0])
    assert type(out.grad_fn).__name__ == '_ConvStemFnBackward'
    g = torch.autograd.grad(out, params, cots[0])
    o64 = ref(xs[0].detach().double().cpu())
    g64 = torch.autograd.grad(o64, list(ref.parameters()), cots[0].double().cpu())
    measure('ConvStem: x [%d, 3, 32, 32] -> 256 filters (7 launches forward, 10 backward)' % a.n,
            {'fused': stem, 'modules': lambda t: nn.Sequential.forward(stem, t)}, xs, cots, lambda name, x: params,
            worst([out] + list(g), [o64] + list(g64)))
    del xs, cots

    # ---- the hand-off of the `ode2` stem ---------------------------------------------------------------------------
    for c, side in ((256, 16), (64, 14)):
        torch.manual_seed(1)
        ode2 = nof.ODEDownsample2(3, c).cuda()
        plain = copy.copy(ode2)            # the same parameters, the module path
        plain.fused_handoff = False
        params = [ode2.norm[0].weight, ode2.norm[0].bias, ode2.conv2.weight, ode2.conv2.bias]
        xs, cots = buffers((a.n, c, side, side), (a.n, c, side // 2, side // 2), True)
        out = ode2._handoff(xs[0])
        assert type(out.grad_fn).__name__ == '_DownConvFnBackward'
        assert type(plain._handoff(xs[0]).grad_fn).__name__ != '_DownConvFnBackward'
        g = torch.autograd.grad(out, params + [xs[0]], cots[0])
        gn64, conv64 = copy.deepcopy(ode2.norm[0]).double().cpu(), copy.deepcopy(ode2.conv2).double().cpu()
        x64 = xs[0].detach().double().cpu().requires_grad_(True)
        o64 = conv64(F.relu(gn64(x64)))
        g64 = torch.autograd.grad(o64, [gn64.weight, gn64.bias, conv64.weight, conv64.bias, x64], cots[0].double().cpu())
        measure('hand-off: x [%d, %d, %d, %d] -> %d filters (5 launches forward, 6 backward)' % (a.n, c, side, side, c),
                {'fused': ode2._handoff, 'modules': plain._handoff}, xs, cots, lambda name, x, params=params: params + [x],
                worst([out] + list(g), [o64] + list(g64)))
        del xs, cots


if __name__ == '__main__':
    main()

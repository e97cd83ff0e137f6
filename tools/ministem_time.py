#!/usr/bin/env python
"""Times of the `minimal` stem (ministem.py) and of the conv stems' input-gradient backward (`input_grad`: node_ministem_bwd,
node_convstem_bwd_dx) against the module sequence they replace -- `nn.Sequential.forward` (MIOpen / ATen) -- in ONE process,
alternating the two:

    python3 tools/ministem_time.py > profiles/ministem_time.txt

Per shape and stem: forward (inference, under no_grad); forward + backward of every parameter; forward + input-gradient backward
with frozen parameters (what an attack or a saliency map runs).  Each is HIP events around a window of `--reps` calls from
Python (what a training step sees: dispatch included), the two paths alternating round by round, median over the rounds.  The
operands of a call -- the input and the output gradient -- ROTATE through enough buffers to exceed the 256 MB Infinity Cache
between two uses of one of them, so they arrive cache-cold; activations live in the workspace (fused) or come from the caching
allocator (modules), the same blocks call after call, for both paths alike.  Next to the times: the device kernels one call
launches on either path (torch.profiler)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 3, 32, 32, 256), (128, 1, 28, 28, 64), (1, 3, 32, 32, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()

    import torch
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

    def buffers(shape_x, shape_c):
        per = 4 * (torch.Size(shape_x).numel() + torch.Size(shape_c).numel())
        nsets = min(4096, max(2, -(-320 * 1000 * 1000 // per)))
        return [torch.randn(shape_x, device='cuda') for _ in range(nsets)], [torch.randn(shape_c, device='cuda') for _ in range(nsets)]

    for kind, cls, node in (('minimal', nof.MinimalStem, '_MiniStemFnBackward'), ('convolution', nof.ConvStem, '_ConvStemFnBackward')):
        for n, cin, h, w, filters in SHAPES:
            torch.manual_seed(0)
            stem = nof.ODENet(cin, n_filters=filters, downsample=kind).downsample.module.cuda()
            assert isinstance(stem, cls)
            stem.input_grad = True
            params = list(stem.parameters())
            paths = {'fused': stem, 'modules': lambda t: nn.Sequential.forward(stem, t)}
            side = lambda s: ((s - 2 - 2) // 2 + 1 - 2) // 2 + 1
            xs, cots = buffers((n, cin, h, w), (n, filters, side(h), side(w)))
            i = [0]

            def nxt():
                i[0] = (i[0] + 1) % len(xs)
                return xs[i[0]], cots[i[0]]

            def fwd(name):
                def fn():
                    with torch.no_grad():
                        paths[name](nxt()[0])
                return fn

            def train(name):
                def fn():
                    x, c = nxt()
                    torch.autograd.grad(paths[name](x), params, c)
                return fn

            def attack(name):
                def fn():
                    x, c = nxt()
                    xg = x.detach().requires_grad_(True)
                    torch.autograd.grad(paths[name](xg), xg, c)
                return fn
            assert type(stem(xs[0]).grad_fn).__name__ == node
            assert type(paths['modules'](xs[0]).grad_fn).__name__ != node
            print('\n%s: x [%d, %d, %d, %d] -> %d filters; operands rotate through %d buffers (%.0f MB)'
                  % (cls.__name__, n, cin, h, w, filters, len(xs), len(xs) * (xs[0].numel() + cots[0].numel()) * 4 / 1e6))
            print('%-44s %10s %11s %7s %s' % ('', 'fused us', 'modules us', 'ratio', '   kernels fused / modules'))
            rows = [('forward (no_grad)', fwd, False), ('forward + backward (parameters)', train, False),
                    ('forward + input-gradient backward (frozen)', attack, True)]
            if kind == 'convolution':      # (its first two rows: tools/convstem_time.py)
                rows = rows[2:]
            for what, make, frozen in rows:
                for p in params:
                    p.requires_grad_(not frozen)
                runs = {p: window(make(p)) for p in paths}
                t = {p: [] for p in runs}
                for _ in range(a.rounds):
                    for p in runs:
                        t[p].append(runs[p]())
                med = {p: statistics.median(v) for p, v in t.items()}
                counts = {p: kernels(make(p)) for p in paths}
                print('%-44s %10.1f %11.1f %7.2f    %s / %s   (min %.1f / %.1f, max %.1f / %.1f)'
                      % (what, med['fused'], med['modules'], med['modules'] / med['fused'], counts['fused'], counts['modules'],
                         min(t['fused']), min(t['modules']), max(t['fused']), max(t['modules'])))
            del xs, cots


if __name__ == '__main__':
    main()

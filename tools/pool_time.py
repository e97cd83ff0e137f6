#!/usr/bin/env python
"""Times of the `ode` stem's hand-off (pool.py: `max_pool_4s2`, `trajectory_pool`) against what it replaces -- `nn.MaxPool2d(4, 2, 1)`
(ATen: forward kernel; backward = zero-fill + atomic scatter) and, in feature extraction, `torch.stack([f.mean(-1).mean(-1) for f in
traj])` next to the max-pool of the last slice -- in ONE process, alternating the two:

    python3 tools/pool_time.py > profiles/pool_time.txt

Per shape: forward (under no_grad), forward + backward (torch.autograd.grad of the input, which the solve in front needs) and the
feature call on a trajectory of `--slices` time points, each as HIP events around a window of `--reps` calls from Python (what a
training step sees: dispatch included), alternating the two paths round by round; median, minimum and maximum over the rounds.
The operands of a call -- the input and the output gradient -- ROTATE through enough buffers to exceed the 256 MB Infinity Cache
between two uses of one of them, so they arrive cache-cold (one trajectory alone exceeds it; two alternate).  Outputs come from
the caching allocator, the same blocks call after call, for both paths alike.  Next to the time of a call: the device time of its
kernels (torch.profiler, 10 calls on the same rotating operands, a run of its own) and GB/s = the bytes the fused kernels must
move (every operand and result once) over that device time, for either path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((128, 256, 16, 16), 'CIFAR at 256 filters'), ((128, 64, 14, 14), 'MNIST'), ((64, 256, 32, 32), '64x64 inputs')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--slices', type=int, default=21)
    a = ap.parse_args()

    import torch
    from torch import nn
    from neural_ode_features_amd import pool
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s; %d calls per timed window, median of %d rounds, paths alternating' % (torch.cuda.get_device_name(0), a.reps, a.rounds))
    module = nn.MaxPool2d(4, 2, 1)

    def window(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()

        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / reps
        return run

    def kernels(fn, calls=10):
        """(device kernels of one call, their device time in us per call) from torch.profiler over `calls` calls with rotating,
        cache-cold operands -- or (None, nan) where the profiler cannot see the device"""
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
            evs = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()]
            if not evs:
                return None, float('nan')
            return len(evs) // calls, sum(e.device_time for e in evs) / calls
        except Exception as exc:       # noqa: BLE001
            print('(no kernel count: %s)' % exc)
            return None, float('nan')

    def report(what, fns, nbytes, reps):
        runs = {p: window(fns[p], reps) for p in fns}
        t = {p: [] for p in runs}
        for _ in range(a.rounds):
            for p in runs:
                t[p].append(runs[p]())
        med = {p: statistics.median(v) for p, v in t.items()}
        (kf, df), (km, dm) = kernels(fns['fused']), kernels(fns['modules'])
        print('%-20s %8.1f %8.1f %6.2f | %8.1f %8.1f %6.2f %7.0f %7.0f | %s / %s   (call min %.1f / %.1f, max %.1f / %.1f)'
              % (what, med['fused'], med['modules'], med['modules'] / med['fused'], df, dm, dm / df, nbytes / df / 1e3, nbytes / dm / 1e3,
                 kf, km, min(t['fused']), min(t['modules']), max(t['fused']), max(t['modules'])))

    for shape, title in SHAPES:
        n, c, h, w = shape
        oh, ow = (h - 2) // 2 + 1, (w - 2) // 2 + 1
        nx, ny = n * c * h * w, n * c * oh * ow
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // (4 * (nx + ny)))))
        torch.manual_seed(0)
        xs = [torch.randn(shape, device='cuda').requires_grad_(True) for _ in range(nsets)]
        cots = [torch.randn(n, c, oh, ow, device='cuda') for _ in range(nsets)]
        i = [0]

        def nxt():
            i[0] = (i[0] + 1) % nsets
            return xs[i[0]], cots[i[0]]

        paths = {'fused': pool.max_pool_4s2, 'modules': module}
        out = pool.max_pool_4s2(xs[0])
        assert type(out.grad_fn).__name__ == '_MaxPool4s2FnBackward' and torch.equal(out, module(xs[0]))

        def fwd(p):
            def fn():
                with torch.no_grad():
                    paths[p](nxt()[0])
            return fn

        def both(p):
            def fn():
                x, g = nxt()
                torch.autograd.grad(paths[p](x), x, g)
            return fn
        print('\n%s: x [%d, %d, %d, %d] -> [%d, %d, %d, %d]; operands rotate through %d buffers (%.0f MB)'
              % ((title,) + shape + (n, c, oh, ow, nsets, nsets * 4 * (nx + ny) / 1e6)))
        print('%-20s %8s %8s %6s | %8s %8s %6s %7s %7s | %s' % ('', 'call us', 'modules', 'ratio', 'kern. us', 'modules', 'ratio', 'GB/s', 'modules', 'kernels'))
        report('forward', {p: fwd(p) for p in paths}, 4 * nx + 4 * ny, a.reps)
        # forward: x in, pooled + argmax out; backward: grad_y + argmax in, d_x out
        report('forward + backward', {p: both(p) for p in paths}, (4 * nx + 5 * ny) + (5 * ny + 4 * nx), a.reps)
        del xs, cots
        torch.cuda.empty_cache()

        t = a.slices
        trajs = [torch.randn((t,) + shape, device='cuda') for _ in range(2)]       # each larger than the Infinity Cache
        k = [0]

        def nxt_traj():
            k[0] ^= 1
            return trajs[k[0]]

        def feat_fused():
            with torch.no_grad():
                pool.trajectory_pool(nxt_traj())

        def feat_modules():
            with torch.no_grad():
                f = nxt_traj()
                torch.stack([fi.mean(-1).mean(-1) for fi in f]), module(f[-1])
        m1, p1 = pool.trajectory_pool(trajs[0])
        assert torch.equal(p1, module(trajs[0][-1]))
        assert torch.allclose(m1, torch.stack([fi.mean(-1).mean(-1) for fi in trajs[0]]), rtol=1e-5, atol=1e-6)
        report('features, %d slices' % t, {'fused': feat_fused, 'modules': feat_modules}, 4 * t * nx + 4 * ny + 4 * t * n * c, max(5, a.reps // 5))
        del trajs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

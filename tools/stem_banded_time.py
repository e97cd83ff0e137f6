#!/usr/bin/env python
"""The residual stem on 64 x 64 images (stem.py `_BandedStemFn`, node_stem_banded_*, csrc/kernels_stem_banded.hip), the HIP node
against the module sequence it replaces, in ONE process, alternating them round by round (the protocol of tools/bnstem_time.py):

    python3 tools/stem_banded_time.py > profiles/stem_banded_time.txt

  fused      `ResidualStem.fused_banded = True`: node_stem_banded_fwd / node_stem_banded_bwd / node_stem_banded_bwd_dx
  modules    the switch off: what ran before the node existed (MIOpen convolutions, ATen group norms, ReLUs, additions)

Timed calls, from Python (dispatch included), at [64, 3, 64, 64] -> 1024 (the per-GPU shape of BASELINE.json configs[4]),
[128, 3, 64, 64] -> 256 and [1, 3, 64, 64] -> 1024: `forward` under no_grad; `forward + backward` (`torch.autograd.grad` with respect
to every parameter); `forward + input-gradient backward` with frozen parameters and `input_grad` on (what `attack.bim` runs).  HIP
events around `--reps` calls, every path warmed up, the paths alternating round by round, median, minimum and spread (max - min)
over `--rounds` rounds.  Input and cotangent ROTATE through enough buffers to exceed the 256 MB Infinity Cache between two uses of
one of them.  The device kernels of ONE call are counted with torch.profiler.

A row is a GAIN when the modules' median minus the fused median exceeds three times the spread of the modules' rounds of the same
run; a row whose fused median is the larger one says SLOWER.  The deciding row for the default of `fused_banded` is forward +
backward at [64, 3, 64, 64] -> 1024.

The band A/B (NODE_TUNE_STEM_BAND_PX, read by the library once per call) on the deciding row: 64, 128 (the default), 256 and 512
pixels per band, alternating round by round in the same process; a height WINS when the default's median minus its median exceeds
three times the spread of the default's rounds.

Then one training step of `bench.py --config 5`'s model (StackedODENet, 1024 filters, three blocks, dopri5 tol 1e-3, 64 images of
64 x 64), fused against modules -- the modules ARE what the commit before this node ran at this shape -- and the library-convolution
kernels (MIOpen's) that are left in a fused step, by name."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((64, 3, 64, 64), 1024), ((128, 3, 64, 64), 256), ((1, 3, 64, 64), 1024)]
BANDS = (128, 64, 256, 512)
ENV = 'NODE_TUNE_STEM_BAND_PX'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-bands', action='store_true')
    a = ap.parse_args()

    import torch
    import neural_ode_features_amd as nof
    from neural_ode_features_amd.head import cross_entropy
    from neural_ode_features_amd.stem import ResidualStem
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s' % torch.cuda.get_device_name(0))
    os.environ.pop(ENV, None)
    default = ResidualStem.fused_banded

    def switched(on, fn):
        def call(*args):
            ResidualStem.fused_banded = on
            try:
                return fn(*args)
            finally:
                ResidualStem.fused_banded = default
        return call

    def timed(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def device_events(step):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return [e for e in prof.key_averages() if e.device_type == DeviceType.CUDA]

    def kernels_of(step):
        try:
            return sum(e.count for e in device_events(step))
        except Exception as exc:      # (no device tracing in this build)
            return 'n/a (%s)' % type(exc).__name__

    def compare(what, fn, reps, rounds, unit=1.0, suffix='us', warm=5):
        steps = {'fused': switched(True, fn), 'modules': switched(False, fn)}
        for s in steps.values():
            for _ in range(warm):
                s()
        torch.cuda.synchronize()
        ts = {k: [] for k in steps}
        for _ in range(rounds):
            for k, s in steps.items():
                ts[k].append(timed(s, reps) / unit)
        med = {k: statistics.median(v) for k, v in ts.items()}
        spread = {k: max(v) - min(v) for k, v in ts.items()}
        for k, s in steps.items():
            print('  %-28s %-8s median %9.2f %s   min %9.2f   spread %8.2f   device kernels per call: %s'
                  % (what, k, med[k], suffix, min(ts[k]), spread[k], kernels_of(s)))
        diff = med['modules'] - med['fused']
        verdict = 'GAIN' if diff > 3 * spread['modules'] else ('SLOWER fused' if diff < 0 else 'no gain by the bar')
        print('  %-28s modules / fused %.2f   difference of the medians %.2f %s against 3 x the modules\' spread %.2f: %s'
              % (what, med['modules'] / med['fused'], diff, suffix, 3 * spread['modules'], verdict), flush=True)

    def stem_of(in_ch, filters):
        torch.manual_seed(0)
        return nof.ODENet(in_ch, out=10, n_filters=filters, downsample='residual', adjoint=True).downsample.module.cuda()

    def calls_of(stem, shape, filters):
        n, cin, h, w = shape
        o = lambda s: ((s - 2 - 1) // 2 + 1 - 1) // 2 + 1
        act = n * 64 * (h - 2) * (w - 2) * 4          # the largest activation: what has to leave the cache between two calls
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // act)))
        xs = [torch.randn(n, cin, h, w, device='cuda') for _ in range(nsets)]
        xg = [x.clone().requires_grad_(True) for x in xs]
        cots = [torch.randn(n, filters, o(h), o(w), device='cuda') for _ in range(nsets)]
        params = list(stem.parameters())
        i = [0]

        def forward():
            i[0] = (i[0] + 1) % nsets
            with torch.no_grad():
                return stem(xs[i[0]])

        def backward():
            i[0] = (i[0] + 1) % nsets
            return torch.autograd.grad(stem(xs[i[0]]), params, cots[i[0]])

        def input_backward():
            i[0] = (i[0] + 1) % nsets
            stem.input_grad = True
            for p in params:
                p.requires_grad_(False)
            try:
                return torch.autograd.grad(stem(xg[i[0]]), [xg[i[0]]], cots[i[0]])
            finally:
                stem.input_grad = False
                for p in params:
                    p.requires_grad_(True)
        return forward, backward, input_backward, i, nsets, act

    for shape, filters in SHAPES:
        n, cin, h, w = shape
        stem = stem_of(cin, filters)
        forward, backward, input_backward, i, nsets, act = calls_of(stem, shape, filters)
        assert type(switched(True, stem)(torch.randn(*shape, device='cuda')).grad_fn).__name__ == '_BandedStemFnBackward'
        print('\nGroupNorm residual stem, x [%d, %d, %d, %d] -> %d filters (largest activation %.2f MB); %d calls per timed window, %d rounds, '
              'input and cotangent rotating through %d sets' % (n, cin, h, w, filters, act / 1e6, a.reps, a.rounds, nsets))
        compare('forward', forward, a.reps, a.rounds)
        compare('forward+backward', backward, a.reps, a.rounds)
        compare('forward+input-grad (frozen)', input_backward, a.reps, a.rounds)

    if not a.no_bands:
        shape, filters = SHAPES[0]
        stem = stem_of(shape[1], filters)
        _, backward, _, i, nsets, _ = calls_of(stem, shape, filters)

        def under(px, fn):
            def call():
                os.environ[ENV] = str(px)
                try:
                    return switched(True, fn)()
                finally:
                    os.environ.pop(ENV, None)
            return call
        steps = {px: under(px, backward) for px in BANDS}
        print('\npixels per band of the banded GroupNorm passes (%s), forward + backward at x [%d, %d, %d, %d] -> %d: %d calls per timed '
              'window, %d rounds, the heights alternating round by round' % ((ENV,) + shape + (filters, a.reps, a.rounds)))
        for s in steps.values():
            for _ in range(5):
                s()
        torch.cuda.synchronize()
        ts = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, s in steps.items():
                ts[k].append(timed(s, a.reps))
        med = {k: statistics.median(v) for k, v in ts.items()}
        spread = {k: max(v) - min(v) for k, v in ts.items()}
        for px in BANDS:
            line = '  band %4d px   forward+backward median %9.2f us   min %9.2f   spread %8.2f' % (px, med[px], min(ts[px]), spread[px])
            if px != BANDS[0]:
                diff = med[BANDS[0]] - med[px]
                line += '   default - this %8.2f us against 3 x the default\'s spread %.2f: %s' % (
                    diff, 3 * spread[BANDS[0]], 'WINS' if diff > 3 * spread[BANDS[0]] else ('slower' if diff < 0 else 'no gain by the bar'))
            print(line)
        print('  device time of the GroupNorm kernels of ONE forward + backward (us; mean over 5 profiled calls; launches per call in brackets):')
        try:
            for px in BANDS:
                def five():
                    for _ in range(5):
                        steps[px]()
                evs = [e for e in device_events(five) if 'k_stem_gn' in e.key]
                tot = lambda e: getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
                name = lambda e: e.key.replace('node::(anonymous namespace)::', '').replace('void ', '').split('(')[0]
                parts = ['%s %.1f [%d]' % (name(e), tot(e) / 5, e.count // 5) for e in sorted(evs, key=name)]
                print('  band %4d px   all %8.1f   %s' % (px, sum(tot(e) for e in evs) / 5, '   '.join(parts)))
        except Exception as exc:      # (no device tracing in this build)
            print('  n/a (%s)' % type(exc).__name__)
        sys.stdout.flush()

    if a.no_step:
        return
    images = torch.randn(64, 3, 64, 64, device='cuda')
    target = torch.randint(0, 10, (64,), device='cuda')
    torch.manual_seed(0)
    model = nof.StackedODENet(3, out=10, n_filters=1024, n_blocks=3, downsample='residual', adjoint=True, tol=1e-3, method='dopri5').cuda()
    opt = nof.FusedSGD(model.parameters(), lr=0.0, momentum=0.9)      # (learning rate 0: every timed step solves the same problem)

    def train_step():
        loss = cross_entropy(model(images), target)
        loss.backward()
        opt.step()
        opt.zero_grad()
    print('\none training step, StackedODENet(3, 1024 filters, 3 blocks, residual stem, adjoint, dopri5 tol 1e-3), batch 64 of 64x64, SGD (lr 0): '
          '2 steps per timed window, %d rounds' % a.rounds)
    compare('configs[4] training step', train_step, 2, a.rounds, unit=1e3, suffix='ms', warm=2)
    try:
        evs = device_events(switched(True, train_step))
        tot = lambda e: getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
        left = [e for e in evs if any(s in e.key.lower() for s in ('igemm', 'miopen', 'sp3asm', 'naive_conv', 'batched_transpose'))]
        print('  library-convolution kernels left in ONE fused step: %s' % (', '.join('%s x %d (%.1f us)' % (e.key[:60], e.count, tot(e)) for e in left) or 'none'))
        print('  device time of one fused step: %.1f ms in %d kernels' % (sum(tot(e) for e in evs) / 1e3, sum(e.count for e in evs)))
    except Exception as exc:
        print('  n/a (%s)' % type(exc).__name__)


if __name__ == '__main__':
    main()

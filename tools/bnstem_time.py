#!/usr/bin/env python
"""The `norm='batch'` residual stem (stem.py `_BnStemFn`, csrc/bnstem_api.hip), the HIP node against the module sequence it
replaces, in ONE process, alternating them round by round:

    python3 tools/bnstem_time.py > profiles/bnstem_time.txt

  fused      `ResidualStem.fused_batch = True`: node_bnstem_fwd / node_bnstem_bwd
  modules    the switch off: what ran before the node existed (MIOpen convolutions, ATen batch norms, ReLUs, additions)

Timed calls, from Python (dispatch included), at [128, 3, 32, 32] -> 256, [128, 1, 28, 28] -> 64 and [1, 3, 32, 32] -> 256: `forward`
under no_grad; `forward + backward` (`torch.autograd.grad` with respect to every parameter); `forward + input-gradient backward`
with frozen parameters and `input_grad` on (what `attack.bim` runs).  Then, at the CIFAR shape, batch 128, SGD: one step of
`train --norm batch -f 256 -a` (dopri5, tol 1e-3, the solve inside the library) and one of `train --model resnet --norm batch -f 256`.
HIP events around `--reps` calls, every path warmed up with 10 calls, the paths alternating round by round, median, minimum and
spread (max - min) over `--rounds` rounds.  Input and cotangent ROTATE through enough buffers to exceed the 256 MB Infinity Cache
between two uses of one of them.  The device kernels of ONE call are counted with torch.profiler.

A row is a GAIN when the modules' median minus the fused median exceeds three times the spread of the modules' rounds of the same
run; a row whose fused median is the larger one says SLOWER.

The chunk-cap A/B (NODE_TUNE_BNSTEM_MAXCHUNK, read by the library once per call): forward + backward at the CIFAR shape under caps
128 (the default: bn_chunk_rows), 256, 512 and 1024, alternating round by round in the same process, and the device time of the
twelve BatchNorm launches of one forward + backward under each cap, kernel by kernel (torch.profiler).  A finer cap WINS when the
default's median minus its median exceeds three times the spread of the default's rounds."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((128, 3, 32, 32), 256), ((128, 1, 28, 28), 64), ((1, 3, 32, 32), 256)]
CAPS = (128, 256, 512, 1024)
ENV = 'NODE_TUNE_BNSTEM_MAXCHUNK'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-caps', action='store_true')
    a = ap.parse_args()

    import torch
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import _lib
    from neural_ode_features_amd.head import cross_entropy
    from neural_ode_features_amd.stem import ResidualStem
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s' % torch.cuda.get_device_name(0))
    os.environ.pop(ENV, None)

    def switched(on, fn):
        def call(*args):
            ResidualStem.fused_batch = on
            try:
                return fn(*args)
            finally:
                ResidualStem.fused_batch = True
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

    def compare(what, fn, reps, rounds, unit=1.0, suffix='us', warm=10):
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
        return nof.ODENet(in_ch, out=10, n_filters=filters, downsample='residual', adjoint=True, norm='batch').downsample.module.cuda()

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
        assert type(stem(torch.randn(*shape, device='cuda')).grad_fn).__name__ == '_BnStemFnBackward'
        # the two paths compute the same thing (biases of every norm at +8: no ReLU mask can differ)
        norms = [m for m in stem.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        with torch.no_grad():
            for m in norms:
                m.bias.add_(8.0)
        worst = {}
        for name, fn in (('parameter gradients', backward), ('image gradient', input_backward)):
            i[0] = 0
            ga = switched(True, fn)()
            i[0] = 0
            gb = switched(False, fn)()
            gmax = max(float(v.abs().max()) for v in gb)
            worst[name] = max(float((u - v).abs().max()) / max(float(v.abs().max()), 1e-4 * gmax) for u, v in zip(ga, gb))
        with torch.no_grad():
            for m in norms:
                m.bias.sub_(8.0)
        print('\nnorm=batch residual stem, x [%d, %d, %d, %d] -> %d filters (largest activation %.2f MB); %d calls per timed window, %d rounds, '
              'input and cotangent rotating through %d sets; fused vs modules, kink-free: worst max-norm difference of the parameter gradients '
              '%.1e, of the image gradient %.1e (relative to max(largest entry, 1e-4 x the largest gradient))'
              % (n, cin, h, w, filters, act / 1e6, a.reps, a.rounds, nsets, worst['parameter gradients'], worst['image gradient']))
        compare('forward', forward, a.reps, a.rounds)
        compare('forward+backward', backward, a.reps, a.rounds)
        compare('forward+input-grad (frozen)', input_backward, a.reps, a.rounds)

    if not a.no_caps:
        shape, filters = SHAPES[0]
        stem = stem_of(shape[1], filters)
        _, backward, _, i, nsets, _ = calls_of(stem, shape, filters)

        def under(cap, fn):
            def call():
                os.environ[ENV] = str(cap)
                try:
                    return fn()
                finally:
                    os.environ.pop(ENV, None)
            return call
        steps = {cap: under(cap, backward) for cap in CAPS}
        print('\nchunk cap of the BatchNorm passes (%s), forward + backward at x [%d, %d, %d, %d] -> %d: %d calls per timed window, %d rounds, '
              'the caps alternating round by round' % ((ENV,) + shape + (filters, a.reps, a.rounds)))
        for cap in CAPS:
            os.environ[ENV] = str(cap)
            plan = _lib.bnstem_plan(*shape, filters)
            os.environ.pop(ENV, None)
            print('  cap %4d: chunks x rows per chunk of the four norms: %s' % (cap, ', '.join('%d x %d (%d tiles)' % (d['nchunk'], d['chunk_rows'], d['column_tiles']) for d in plan)))
        for s in steps.values():
            for _ in range(10):
                s()
        torch.cuda.synchronize()
        ts = {k: [] for k in steps}
        for _ in range(a.rounds):
            for k, s in steps.items():
                ts[k].append(timed(s, a.reps))
        med = {k: statistics.median(v) for k, v in ts.items()}
        spread = {k: max(v) - min(v) for k, v in ts.items()}
        for cap in CAPS:
            line = '  cap %4d   forward+backward median %9.2f us   min %9.2f   spread %8.2f' % (cap, med[cap], min(ts[cap]), spread[cap])
            if cap != CAPS[0]:
                diff = med[CAPS[0]] - med[cap]
                line += '   default - this %8.2f us against 3 x the default\'s spread %.2f: %s' % (
                    diff, 3 * spread[CAPS[0]], 'WINS' if diff > 3 * spread[CAPS[0]] else ('slower' if diff < 0 else 'no gain by the bar'))
            print(line)
        # the twelve BatchNorm launches of one forward + backward, kernel by kernel (device time, us; mean of 5 calls)
        print('  device time of the BatchNorm kernels of ONE forward + backward (us; mean over 5 profiled calls; launches per call in brackets):')
        try:
            for cap in CAPS:
                def five():
                    for _ in range(5):
                        steps[cap]()
                evs = [e for e in device_events(five) if 'k_bn_' in e.key]
                tot = lambda e: getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
                name = lambda e: e.key.replace('node::(anonymous namespace)::', '').replace('void ', '').split('(')[0]
                parts = ['%s %.1f [%d]' % (name(e), tot(e) / 5, e.count // 5) for e in sorted(evs, key=name)]
                print('  cap %4d   all twelve %8.1f   %s' % (cap, sum(tot(e) for e in evs) / 5, '   '.join(parts)))
        except Exception as exc:      # (no device tracing in this build)
            print('  n/a (%s)' % type(exc).__name__)
        sys.stdout.flush()

    if a.no_step:
        return
    images = torch.randn(128, 3, 32, 32, device='cuda')
    target = torch.randint(0, 10, (128,), device='cuda')

    def step_of(model):
        opt = nof.FusedSGD(model.parameters(), lr=0.0, momentum=0.9)      # (learning rate 0: every timed step solves the same problem)

        def train_step():
            loss = cross_entropy(model(images), target)
            loss.backward()
            opt.step()
            opt.zero_grad()
        return train_step
    torch.manual_seed(0)
    model = nof.ODENet(3, n_filters=256, downsample='residual', norm='batch', adjoint=True, tol=1e-3, method='dopri5').cuda()
    for m in model.modules():
        if isinstance(m, nof.ODEfunc):
            m.batch_solve = True          # (what the command line switches on: resnet.build_model)
    print('\none training step, ODENet(3, 256 filters, residual stem, norm=batch, adjoint, dopri5 tol 1e-3, the solve inside the library), '
          'batch 128 of 32x32, SGD (lr 0): 5 steps per timed window, %d rounds' % a.rounds)
    compare('train --norm batch -a', step_of(model), 5, a.rounds, unit=1e3, suffix='ms', warm=3)
    del model
    torch.manual_seed(0)
    model = nof.ResNet(3, n_filters=256, downsample='residual', norm='batch').cuda()
    print('\none training step, ResNet(3, 256 filters, residual stem, norm=batch), batch 128 of 32x32, SGD (lr 0): 5 steps per timed window, '
          '%d rounds' % a.rounds)
    compare('train --model resnet', step_of(model), 5, a.rounds, unit=1e3, suffix='ms', warm=3)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""The `norm='batch'` minimal stem (ministem.py `_BnMiniStemFn`, csrc/bnministem_api.hip), the HIP node against the module sequence
it replaces, in ONE process, alternating them round by round:

    python3 tools/bnministem_time.py > profiles/bnministem_time.txt

  fused      `MinimalStem.fused_batch = True`: node_bnministem_fwd / node_bnministem_bwd
  modules    the switch off: what ran before the node existed (MIOpen convolutions, ATen batch norms, ReLUs)

Timed calls, from Python (dispatch included):
  the stem at [128, 3, 32, 32] -> 256, [128, 1, 28, 28] -> 64 and [1, 3, 32, 32] -> 256: `forward` under no_grad; `forward + backward`
    (`torch.autograd.grad` with respect to every parameter); `forward + input-gradient backward` with frozen parameters and
    `input_grad` on (what `attack.bim` runs);
  at the CIFAR shape, batch 128, SGD: one step of `train --norm batch -d minimal -f 256 -a` (dopri5, tol 1e-3, the solve inside the
    library).
HIP events around `--reps` calls, every path warmed up with 10 calls, the paths alternating round by round, median, minimum and
spread (max - min) over `--rounds` rounds.  Input and cotangent ROTATE through enough buffers to exceed the 256 MB Infinity Cache
between two uses of one of them.  The device kernels of ONE call are counted with torch.profiler.

A row is a GAIN when the modules' median minus the fused median exceeds three times the spread of the modules' rounds of the same
run; a row whose fused median is the larger one says SLOWER."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEM_SHAPES = [((128, 3, 32, 32), 256), ((128, 1, 28, 28), 64), ((1, 3, 32, 32), 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()

    import torch
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import _lib
    from neural_ode_features_amd.head import cross_entropy
    from neural_ode_features_amd.ministem import MinimalStem
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s' % torch.cuda.get_device_name(0))
    default = MinimalStem.fused_batch
    print('MinimalStem.fused_batch ships %s' % default)
    # the cap on the chunks of a BatchNorm pass: the built-in 128 unless the run is about another one
    print('NODE_TUNE_BNMINI_MAXCHUNK: %s; plan at %s -> %d: %s' % (os.environ.get('NODE_TUNE_BNMINI_MAXCHUNK', 'unset'), STEM_SHAPES[0][0], STEM_SHAPES[0][1], [
        (d['rows'], d['chunk_rows'], d['nchunk']) for d in _lib.bnministem_plan(*STEM_SHAPES[0][0], STEM_SHAPES[0][1])]))

    def switched(on, fn):
        def call(*args):
            MinimalStem.fused_batch = on
            try:
                return fn(*args)
            finally:
                MinimalStem.fused_batch = default
        return call

    def timed(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def kernels_of(step):
        try:
            from torch.autograd import DeviceType
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            return sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA)
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

    def worst_difference(fn, i):
        """fused against modules on the same operands, kink-free: the worst max-norm difference relative to max(largest entry, 1e-4 x
        the largest of all)"""
        i[0] = 0
        ga = switched(True, fn)()
        i[0] = 0
        gb = switched(False, fn)()
        gmax = max(float(v.abs().max()) for v in gb)
        return max(float((u - v).abs().max()) / max(float(v.abs().max()), 1e-4 * gmax) for u, v in zip(ga, gb))

    def sets_for(nbytes):
        return min(64, max(2, -(-320 * 1000 * 1000 // nbytes)))

    for shape, filters in STEM_SHAPES:
        n, cin, h, w = shape
        torch.manual_seed(0)
        stem = nof.ODENet(cin, out=10, n_filters=filters, downsample='minimal', adjoint=True, norm='batch').downsample.module.cuda()
        o = lambda s: ((s - 2 - 2) // 2 + 1 - 2) // 2 + 1
        act = n * 24 * (h - 2) * (w - 2) * 4          # the largest activation: what has to leave the cache between two calls
        nsets = sets_for(act)
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
        assert type(switched(True, lambda: stem(xs[0]))().grad_fn).__name__ == '_BnMiniStemFnBackward'
        assert type(switched(False, lambda: stem(xs[0]))().grad_fn).__name__ != '_BnMiniStemFnBackward'
        norms = [m for m in stem.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        with torch.no_grad():
            for m in norms:
                m.bias.add_(8.0)          # no ReLU mask can differ between the two paths
        # (the two bias gradients in front of a BatchNorm are zero identically: 1e-4 x the largest gradient is their scale)
        wp, wx = worst_difference(backward, i), worst_difference(input_backward, i)
        with torch.no_grad():
            for m in norms:
                m.bias.sub_(8.0)
        print('\nnorm=batch minimal stem, x [%d, %d, %d, %d] -> %d filters (largest activation %.2f MB); %d calls per timed window, %d rounds, '
              'input and cotangent rotating through %d sets; fused vs modules, kink-free: worst max-norm difference of the parameter gradients '
              '%.1e, of the image gradient %.1e (relative to max(largest entry, 1e-4 x the largest gradient))'
              % (n, cin, h, w, filters, act / 1e6, a.reps, a.rounds, nsets, wp, wx))
        compare('forward', forward, a.reps, a.rounds)
        compare('forward+backward', backward, a.reps, a.rounds)
        compare('forward+input-grad (frozen)', input_backward, a.reps, a.rounds)
        del xs, xg, cots, stem

    if a.no_step:
        return
    images = torch.randn(128, 3, 32, 32, device='cuda')
    target = torch.randint(0, 10, (128,), device='cuda')
    torch.manual_seed(0)
    model = nof.ODENet(3, n_filters=256, downsample='minimal', norm='batch', adjoint=True, tol=1e-3, method='dopri5').cuda()
    for m in model.modules():
        if isinstance(m, nof.ODEfunc):
            m.batch_solve = True          # (what the command line switches on: resnet.build_model)
    opt = nof.FusedSGD(model.parameters(), lr=0.0, momentum=0.9)      # (learning rate 0: every timed step solves the same problem)

    def train_step():
        loss = cross_entropy(model(images), target)
        loss.backward()
        opt.step()
        opt.zero_grad()
    print('\none training step, ODENet(3, 256 filters, minimal stem, norm=batch, adjoint, dopri5 tol 1e-3, the solve inside the library), '
          'batch 128 of 32x32, SGD (lr 0): %d steps per timed window, %d rounds' % (a.reps, a.rounds))
    compare('train -d minimal -a', train_step, a.reps, a.rounds, unit=1e3, suffix='ms', warm=3)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""The `norm='batch'` residual trunk (resnet.py `_BnTrunkFn`, csrc/bntrunk_api.hip) and classifier head (head.py `bn_head_pool`,
csrc/kernels_bnhead.hip), the HIP nodes against the module sequences they replace, in ONE process, alternating them round by round:

    python3 tools/bntrunk_time.py > profiles/bntrunk_time.txt

  fused      `ResidualTrunk.fused_batch = FCClassifier.fused_batch = True`: node_bntrunk_fwd / _bwd, node_bnhead_fwd / _bwd
  modules    both switches off: what ran before the nodes existed (ATen batch norms, MIOpen convolutions, ReLUs, additions, pooling)

Timed calls, from Python (dispatch included): the six-block trunk and the head (`FCClassifier.forward`, its Linear layer included:
the same launch on both paths), each as `forward` under no_grad and as `forward + backward` (`torch.autograd.grad` with respect to
the input and every parameter), at the two workload shapes; then one training step of `train --model resnet --norm batch -f 256`
at the CIFAR shape (batch 128, SGD).  HIP events around `--reps` calls, every path warmed up with 10 calls, the paths alternating
round by round, median, minimum and spread (max - min) over `--rounds` rounds.  Input and cotangent ROTATE through enough buffers to
exceed the 256 MB Infinity Cache between two uses of one of them.  The device kernels of ONE call are counted with torch.profiler.

A row is a GAIN when the modules' median minus the fused median exceeds three times the spread of the modules' rounds of the same
run; a row whose fused median is the larger one says SLOWER."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 256, 8, 8), (128, 64, 7, 7)]      # CIFAR-10 and MNIST behind the residual stem (reproduce.sh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()

    import torch
    import neural_ode_features_amd as nof
    from neural_ode_features_amd.head import cross_entropy
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s' % torch.cuda.get_device_name(0))

    def switched(on, fn):
        def call(*args):
            nof.ResidualTrunk.fused_batch = nof.FCClassifier.fused_batch = on
            try:
                return fn(*args)
            finally:
                nof.ResidualTrunk.fused_batch = nof.FCClassifier.fused_batch = True
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
            print('  %-20s %-8s median %9.2f %s   min %9.2f   spread %8.2f   device kernels per call: %s'
                  % (what, k, med[k], suffix, min(ts[k]), spread[k], kernels_of(s)))
        diff = med['modules'] - med['fused']
        verdict = 'GAIN' if diff > 3 * spread['modules'] else ('SLOWER fused' if diff < 0 else 'no gain by the bar')
        print('  %-20s modules / fused %.2f   difference of the medians %.2f %s against 3 x the modules\' spread %.2f: %s'
              % (what, med['modules'] / med['fused'], diff, suffix, 3 * spread['modules'], verdict))

    for shape in SHAPES:
        n, c, h, w = shape
        torch.manual_seed(0)
        trunk = nof.ResidualTrunk(c, 6, norm='batch').cuda()
        clf = nof.FCClassifier(c, norm='batch').cuda()
        nbytes = n * c * h * w * 4
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // nbytes)))
        xs = [torch.randn(n, c, h, w, device='cuda').requires_grad_(True) for _ in range(nsets)]
        cots = [torch.randn(n, c, h, w, device='cuda') for _ in range(nsets)]
        hcots = [torch.randn(n, 10, device='cuda') for _ in range(nsets)]
        assert type(trunk(xs[0]).grad_fn).__name__ == '_BnTrunkFnBackward'
        assert type(clf.pooled(xs[0]).grad_fn).__name__ == '_BnHeadPoolBackward'
        i = [0]

        def both(mod, cotangents):
            params = list(mod.parameters())

            def forward():
                i[0] = (i[0] + 1) % nsets
                with torch.no_grad():
                    return mod(xs[i[0]])

            def backward():
                i[0] = (i[0] + 1) % nsets
                x = xs[i[0]]
                return torch.autograd.grad(mod(x), [x] + params, cotangents[i[0]])
            return forward, backward
        # the two paths compute the same thing (biases of every norm at +8: no ReLU mask can differ)
        worst = {}
        for name, mod, cotangents in (('trunk', trunk, cots), ('head', clf, hcots)):
            norms = [m for m in mod.modules() if isinstance(m, torch.nn.BatchNorm2d)]
            with torch.no_grad():
                for m in norms:
                    m.bias.add_(8.0)
            _, bwd = both(mod, cotangents)
            i[0] = 0
            ga = switched(True, bwd)()
            i[0] = 0
            gb = switched(False, bwd)()
            worst[name] = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(ga, gb))
            with torch.no_grad():
                for m in norms:
                    m.bias.sub_(8.0)
        print('\nnorm=batch, x [%d, %d, %d, %d] (%.2f MB); %d calls per timed window, %d rounds, input and cotangent rotating through %d '
              'buffers (%.0f MB each way); fused vs modules, kink-free: worst max-norm difference of the input and parameter gradients '
              'trunk %.1e, head %.1e of the largest entry' % (n, c, h, w, nbytes / 1e6, a.reps, a.rounds, nsets, nsets * nbytes / 1e6, worst['trunk'], worst['head']))
        for name, mod, cotangents in (('trunk', trunk, cots), ('head', clf, hcots)):
            fwd, bwd = both(mod, cotangents)
            compare(name + ' forward', fwd, a.reps, a.rounds)
            compare(name + ' forward+backward', bwd, a.reps, a.rounds)

    if a.no_step:
        return
    torch.manual_seed(0)
    model = nof.ResNet(3, n_filters=256, downsample='residual', norm='batch').cuda()
    opt = nof.FusedSGD(model.parameters(), lr=0.0, momentum=0.9)      # (learning rate 0: every timed step solves the same problem)
    images = torch.randn(128, 3, 32, 32, device='cuda')
    target = torch.randint(0, 10, (128,), device='cuda')

    def train_step():
        loss = cross_entropy(model(images), target)
        loss.backward()
        opt.step()
        opt.zero_grad()
    print('\none training step, ResNet(3, 256 filters, residual stem, norm=batch), batch 128 of 32x32, SGD (lr 0): 5 steps per timed window, '
          '%d rounds (the stem is the module sequence on both paths)' % a.rounds)
    compare('training step', train_step, 5, a.rounds, unit=1e3, suffix='ms', warm=3)


if __name__ == '__main__':
    main()

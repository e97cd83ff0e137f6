#!/usr/bin/env python
"""One evaluation of the `norm='batch'` dynamics, `ODEfunc(C, norm='batch')(t, x)` (bnfunc.py, csrc/bnfunc_api.hip), the
HIP node against the module operations it replaces, in ONE process, alternating them round by round:

    python3 tools/bnfunc_time.py > profiles/bnfunc_time.txt

  fused      `ODEfunc.forward` with `ODEfunc.fused_batch = True`: one autograd node, node_bnfunc_fwd / node_bnfunc_bwd
  modules    the same call with the switch off (what ran before the node existed, and what runs for shapes the kernels
             refuse): three ATen batch norms, two MIOpen convolutions over `cat([t * 1, x])`, ReLUs

Timed calls, from Python (what the generic solver sees: dispatch included): `forward` under no_grad (an evaluation of the
forward solve), and `forward + VJP`: a forward and `torch.autograd.grad` of the output with respect to t, x and the ten
parameters (an evaluation of the adjoint solve).  HIP events around `--reps` calls, every path warmed up with 10 calls,
the paths alternating round by round, median and minimum over `--rounds` rounds.  Input and cotangent ROTATE through enough
buffers to exceed the 256 MB Infinity Cache between two uses of one of them.  The device kernels of ONE call are counted
with torch.profiler.  Last, one training step of `train --norm batch -f 256 -a` at the CIFAR shape (dopri5, tol 1e-3, batch
128, SGD) with the switch on and off, alternating."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 256, 8, 8), (128, 64, 7, 7), (1, 256, 8, 8)]      # CIFAR-10 and MNIST behind the residual stem; one image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
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
            nof.ODEfunc.fused_batch = on
            try:
                return fn(*args)
            finally:
                nof.ODEfunc.fused_batch = True
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

    for shape in SHAPES:
        n, c, h, w = shape
        torch.manual_seed(0)
        func = nof.ODEfunc(c, norm='batch').cuda()
        params = list(func.parameters())
        nbytes = n * c * h * w * 4
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // nbytes)))
        xs = [torch.randn(n, c, h, w, device='cuda').requires_grad_(True) for _ in range(nsets)]
        cots = [torch.randn(n, c, h, w, device='cuda') for _ in range(nsets)]
        t = torch.tensor(0.37, device='cuda').requires_grad_(True)
        assert type(func(t, xs[0]).grad_fn).__name__ == '_BatchOdeFnBackward'
        i = [0]

        def forward():
            i[0] = (i[0] + 1) % nsets
            with torch.no_grad():
                return func(t, xs[i[0]])

        def vjp():
            i[0] = (i[0] + 1) % nsets
            x = xs[i[0]]
            return torch.autograd.grad(func(t, x), [t, x] + params, cots[i[0]])
        # the two paths compute the same thing (biases of norm1 / norm2 at +8: no ReLU mask can differ)
        with torch.no_grad():
            func.norm1.bias.add_(8.0)
            func.norm2.bias.add_(8.0)
        i[0] = 0
        ga = switched(True, vjp)()
        i[0] = 0
        gb = switched(False, vjp)()
        worst = max(float((u - v).abs().max() / v.abs().max()) for k, (u, v) in enumerate(zip(ga, gb)) if k not in (5, 9))   # (not the conv biases: zero gradients)
        with torch.no_grad():
            func.norm1.bias.sub_(8.0)
            func.norm2.bias.sub_(8.0)
        print('\nODEfunc(%d, norm=batch), x [%d, %d, %d, %d] (%.2f MB); %d calls per timed window, %d rounds, input and cotangent rotating through '
              '%d buffers (%.0f MB each way); fused vs modules, kink-free: worst max-norm difference of t, x and parameter gradients %.1e of the largest entry'
              % (c, n, c, h, w, nbytes / 1e6, a.reps, a.rounds, nsets, nsets * nbytes / 1e6, worst))
        for what, fn in (('forward', forward), ('forward + VJP', vjp)):
            steps = {'fused': switched(True, fn), 'modules': switched(False, fn)}
            for s in steps.values():
                for _ in range(10):
                    s()
            torch.cuda.synchronize()
            ts = {k: [] for k in steps}
            for _ in range(a.rounds):
                for k, s in steps.items():
                    ts[k].append(timed(s, a.reps))
            med = {k: statistics.median(v) for k, v in ts.items()}
            for k, s in steps.items():
                print('  %-14s %-8s median %8.1f us   min %8.1f us   device kernels per call: %s' % (what, k, med[k], min(ts[k]), kernels_of(s)))
            print('  %-14s modules / fused %.2f' % (what, med['modules'] / med['fused']))

    if a.no_step:
        return
    torch.manual_seed(0)
    model = nof.ODENet(3, n_filters=256, downsample='residual', norm='batch', adjoint=True, tol=1e-3, method='dopri5').cuda()
    opt = nof.FusedSGD(model.parameters(), lr=0.0, momentum=0.9)      # (learning rate 0: every timed step solves the same problem)
    images = torch.randn(128, 3, 32, 32, device='cuda')
    target = torch.randint(0, 10, (128,), device='cuda')
    nfe = {}

    def train_step():
        loss = cross_entropy(model(images), target)
        nf = model.nfe(reset=True)
        loss.backward()
        nb = model.nfe(reset=True)
        opt.step()
        opt.zero_grad()
        return nf, nb
    steps = {'fused': switched(True, train_step), 'modules': switched(False, train_step)}
    for k, s in steps.items():
        for _ in range(3):
            nfe[k] = s()
    torch.cuda.synchronize()
    ts = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            ts[k].append(timed(s, 3))
    print('\none training step, ODENet(3, 256 filters, residual stem, norm=batch, adjoint, dopri5 tol 1e-3), batch 128 of 32x32, SGD (lr 0): '
          '3 steps per timed window, 5 rounds')
    for k in steps:
        print('  %-8s median %8.2f ms   min %8.2f ms   NFE forward / backward %d / %d' % (k, statistics.median(ts[k]) / 1e3, min(ts[k]) / 1e3, nfe[k][0], nfe[k][1]))
    print('  modules / fused %.2f' % (statistics.median(ts['modules']) / statistics.median(ts['fused'])))


if __name__ == '__main__':
    main()

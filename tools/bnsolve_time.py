#!/usr/bin/env python
"""A whole solve of the `norm='batch'` dynamics inside the library (bnsolve.py, csrc/bnsolve_api.hip) against the generic solver
on the node (generic.py around bnfunc.py: what ran before, and what runs with `ODEfunc.batch_solve = False`), in ONE process,
alternating them round by round:

    python3 tools/bnsolve_time.py > profiles/bnsolve_time.txt

  batch      `odeint_adjoint` with `func.batch_solve = True`: node_bnsolve_fwd / node_bnsolve_adjoint
  generic    the same call with the switch off

Timed calls, from Python: the forward solve under no_grad, and forward + adjoint (dopri5, rtol = atol = 1e-3, t = (0, 1)).
HIP events around `--reps` solves, every path warmed up (which also teaches both their step hints), the paths alternating
round by round, median, minimum and spread (max - min) over `--rounds` rounds.  The state and the cotangent ROTATE through
enough buffers to exceed the 256 MB Infinity Cache between two uses of one of them.  Device kernels of ONE solve are counted with
torch.profiler (memory copies and fills are not kernels and are not counted; the larger of three traces, because the tracer
drops records of some short windows) and divided by the evaluations of the dynamics the solve made (`func.nfe`).  Last, one training step of `train --norm batch -f 256 -a` at the CIFAR shape (batch 128, SGD) with the
switch on and off, alternating.

A row is called a GAIN only if the difference of the medians exceeds three times the spread of the generic path's rounds in
this run; otherwise "no loss" or "slower", whichever the figures say."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 256, 8, 8), (128, 64, 7, 7), (1, 256, 8, 8)]      # CIFAR-10 and MNIST behind the residual stem; one image


def verdict(med_new, med_old, old_rounds):
    spread = max(old_rounds) - min(old_rounds)
    diff = med_old - med_new
    if diff > 3 * spread:
        return 'GAIN', spread
    return ('no loss' if diff >= -3 * spread else 'slower'), spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    assert a.rounds >= 7, 'at least 7 rounds'

    import torch
    import neural_ode_features_amd as nof
    from neural_ode_features_amd.head import cross_entropy
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s' % torch.cuda.get_device_name(0))

    def timed(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def kernels_of(step):
        # the tracer drops records of some short windows (a 5 ms forward solve has shown 53 to 283 kernels for the same 283
        # launches): a loss only lowers the count, so the larger of three traces is kept
        try:
            from torch.autograd import DeviceType
            from torch.profiler import ProfilerActivity, profile
            counts = []
            for _ in range(3):
                torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    step()
                    torch.cuda.synchronize()
                counts.append(sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA and 'mem' not in e.key.lower()))
            return max(counts)
        except Exception:      # (no device tracing in this build)
            return None

    def report(what, ts, extra):
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k in ts:
            print('  %-18s %-8s median %8.3f ms   min %8.3f ms   spread %6.3f ms   %s' % (what, k, med[k], min(ts[k]), max(ts[k]) - min(ts[k]), extra[k]))
        word, spread = verdict(med['batch'], med['generic'], ts['generic'])
        print('  %-18s generic / batch %.3f   difference of the medians %+.3f ms against 3 x %.3f ms spread of generic: %s'
              % (what, med['generic'] / med['batch'], med['generic'] - med['batch'], spread, word))

    t = torch.tensor([0.0, 1.0], device='cuda')
    for shape in SHAPES:
        n, c, h, w = shape
        torch.manual_seed(0)
        func = nof.ODEfunc(c, norm='batch').cuda()
        nbytes = n * c * h * w * 4
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // nbytes)))
        ys = [torch.randn(n, c, h, w, device='cuda').requires_grad_(True) for _ in range(nsets)]
        cots = [torch.randn(2, n, c, h, w, device='cuda') / (c * h * w) ** 0.5 for _ in range(nsets)]
        i = [0]

        def forward():
            i[0] = (i[0] + 1) % nsets
            with torch.no_grad():
                return nof.odeint_adjoint(func, ys[i[0]], t, rtol=1e-3, atol=1e-3, method='dopri5')

        def both():
            i[0] = (i[0] + 1) % nsets
            for p in func.parameters():
                p.grad = None
            ys[i[0]].grad = None
            nof.odeint_adjoint(func, ys[i[0]], t, rtol=1e-3, atol=1e-3, method='dopri5').backward(cots[i[0]])

        def switched(on, fn):
            def call():
                func.batch_solve = on
                return fn()
            return call
        print('\nODEfunc(%d, norm=batch), state [%d, %d, %d, %d] (%.2f MB), dopri5 tol 1e-3, t = (0, 1); %d solves per timed window, %d rounds, '
              'state and cotangent rotating through %d buffers' % (c, n, c, h, w, nbytes / 1e6, a.reps, a.rounds, nsets))
        for what, fn in (('forward solve', forward), ('forward + adjoint', both)):
            steps = {'batch': switched(True, fn), 'generic': switched(False, fn)}
            for s in steps.values():
                for _ in range(max(3, nsets // 8)):
                    s()
            torch.cuda.synchronize()
            ts = {k: [] for k in steps}
            for _ in range(a.rounds):
                for k, s in steps.items():
                    ts[k].append(timed(s, a.reps))
            extra = {}
            for k, s in steps.items():
                kn = kernels_of(s)
                func.nfe = 0
                s()
                nfe = func.nfe
                extra[k] = 'NFE %d, device kernels per solve %s = %s per evaluation' % (nfe, kn, 'n/a' if kn is None else '%.1f' % (kn / max(nfe, 1)))
                if kn is not None and kn < 8 * nfe:      # (the passes and convolutions alone are 8 launches per evaluation)
                    extra[k] += ' (TRACE INCOMPLETE)'
            report(what, ts, extra)
        del ys, cots

    if a.no_step:
        return
    torch.manual_seed(0)
    model = nof.ODENet(3, n_filters=256, downsample='residual', norm='batch', adjoint=True, tol=1e-3, method='dopri5').cuda()
    funcs = [m for m in model.modules() if isinstance(m, nof.ODEfunc)]
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

    def switched_step(on):
        def call():
            for f in funcs:
                f.batch_solve = on
            return train_step()
        return call
    steps = {'batch': switched_step(True), 'generic': switched_step(False)}
    for k, s in steps.items():
        for _ in range(3):
            nfe[k] = s()
    torch.cuda.synchronize()
    ts = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, s in steps.items():
            ts[k].append(timed(s, 10))
    print('\none training step, ODENet(3, 256 filters, residual stem, norm=batch, adjoint, dopri5 tol 1e-3), batch 128 of 32x32, SGD (lr 0): '
          '10 steps per timed window, %d rounds' % a.rounds)
    extra = {}
    for k, s in steps.items():
        kn = kernels_of(s)
        ev = nfe[k][0] + nfe[k][1]
        extra[k] = 'NFE forward / backward %d / %d, device kernels per step %s = %s per evaluation' % (
            nfe[k][0], nfe[k][1], kn, 'n/a' if kn is None else '%.1f' % (kn / max(ev, 1)))
    report('training step', ts, extra)


if __name__ == '__main__':
    main()

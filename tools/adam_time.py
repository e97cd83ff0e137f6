#!/usr/bin/env python
"""Time of one Adam step over the parameter set of BASELINE configs[1] (CIFAR-10 ODE-ResNet, 256 filters), by HIP events around
`optimizer.step()`, for three implementations stepped in turn in one process on their own copies of the parameters, with the
same gradients:

    torch    torch.optim.Adam(params, lr, weight_decay=wd) with its defaults -- what `train.py -o adam` ran before FusedAdam
             (on the device PyTorch picks its foreach implementation: a chain of ATen launches; the step counts are CPU
             tensors read on the host)
    fused    torch.optim.Adam(..., fused=True)
    ours     optim.FusedAdam: node_adam_step, two launches

    python3 tools/adam_time.py [--iters 100] [--warmup 20]
    rocprofv3 --kernel-trace --stats -d /tmp/adam -o adam -- python3 tools/adam_time.py    # k_adam_multi's own duration

Events on an otherwise idle stream: a figure holds the launches' host time wherever the host is slower than the device.  The
second column is the host's time to enqueue the step.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    if a.iters < 50:
        raise SystemExit('a median of fewer than 50 steps is not reported')
    import torch
    import bench
    import neural_ode_features_amd as nof
    dev = torch.device('cuda', 0)
    model = bench.build_model(dev, dict(bench.CONFIGS[2]), 'dopri5')     # bench.CONFIGS is keyed 1-based: 2 = BASELINE configs[1]
    source = [p.detach() for p in model.parameters()]
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [1e-2 * torch.randn(p.shape, generator=gen, device=dev) for p in source]

    def copies():
        ps = [p.clone().requires_grad_(True) for p in source]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    opts = [('torch', torch.optim.Adam(copies(), lr=1e-3, weight_decay=1e-4)),
            ('fused', torch.optim.Adam(copies(), lr=1e-3, weight_decay=1e-4, fused=True)),
            ('ours', nof.FusedAdam(copies(), lr=1e-3, weight_decay=1e-4))]
    device_us = {k: [] for k, _ in opts}
    host_us = {k: [] for k, _ in opts}
    for i in range(a.warmup + a.iters):
        for name, opt in opts:                      # in turn: what the box does to one it does to all three
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            opt.step()
            e1.record()
            t1 = time.perf_counter()
            e1.synchronize()
            if i >= a.warmup:
                device_us[name].append(e0.elapsed_time(e1) * 1e3)
                host_us[name].append((t1 - t0) * 1e6)
    n = sum(p.numel() for p in source)
    print('Adam step over %d tensors, %d parameters (%.1f MB read + written at 28 B each), median of %d steps after %d:'
          % (len(source), n, 28e-6 * n, a.iters, a.warmup))
    for name, _ in opts:
        d = device_us[name]
        print('  %-6s events %8.1f us (min %.1f, max %.1f)   host enqueue %8.1f us'
              % (name, statistics.median(d), min(d), max(d), statistics.median(host_us[name])), flush=True)
    ours, parent = statistics.median(device_us['ours']), statistics.median(device_us['torch'])
    print('FusedAdam / parent path: %.3f' % (ours / parent))
    return 0 if ours < parent else 1


if __name__ == '__main__':
    sys.exit(main())

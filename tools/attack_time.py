#!/usr/bin/env python
"""Timings of the adversarial-attack path (README row "attack", DESIGN.md "Input gradient of the residual stem"):

  1. the stem's backward at [B, 3, 32, 32], 256 filters: node_stem_bwd_dx with grads = NULL (input gradient alone) against
     node_stem_bwd (parameter gradients, no input gradient) and against the module-sequence backward with an input gradient
     (what an input that requires a gradient runs without `ResidualStem.input_grad`);
  2. k_stem_conv0_dgrad alone (device time from the profiler's kernel records) against the bytes it must move: dh0 once plus
     the image;
  3. one whole attack iteration (forward solve, loss, adjoint solve, stem backward, step, judge) on the library's path against
     the same loop in plain torch on the default path (`bim_reference` on device tensors, module-sequence stem);
  4. the dopri5 input gradient at the shape of tests/test_gpu_attack.py: the default path against the oracle's fp32 CPU run, and
     the fused-stem path against the default path (the numbers the test's bound is made of).

Device events, warmed up, the variants alternating in one process.

    python tools/attack_time.py [--batches 128 1] [--reps 20] > profiles/attack_time.txt
"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CIFAR = ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))


def _timed(fn, prepare=None):
    """Device milliseconds of fn() (prepare() runs untimed in front of it)."""
    if prepare is not None:
        prepare()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(variants, reps, warm=3):
    """{name: median ms}; variants: {name: (prepare, fn)} run in turn, `reps` rounds after `warm` untimed ones."""
    times = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, (prepare, fn) in variants.items():
            t = _timed(fn, prepare)
            if r >= warm:
                times[k].append(t)
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def stem_backward(batch, reps):
    import neural_ode_features_amd as nof
    torch.manual_seed(0)
    stem = nof.ODENet(3, out=10, n_filters=256, downsample='residual', adjoint=True).downsample.module.cuda()
    x = torch.rand(batch, 3, 32, 32, device='cuda')
    state = {}

    def prep(input_grad, want_x, want_p):
        def go():
            stem.input_grad = input_grad
            for p in stem.parameters():
                p.requires_grad_(want_p)
                p.grad = None
            xin = x.clone().requires_grad_(want_x)
            state['out'] = stem(xin)
            state['cot'] = torch.ones_like(state['out'])
        return go

    def bwd():
        state['out'].backward(state['cot'])
    res = _alternate({'bwd_dx, grads NULL (input gradient only)': (prep(True, True, False), bwd),
                      'bwd_dx with grads (both)': (prep(True, True, True), bwd),
                      'node_stem_bwd (parameter gradients only)': (prep(False, False, True), bwd),
                      'module sequence, input gradient only': (prep(False, True, False), bwd),
                      'module sequence, both': (prep(False, True, True), bwd)}, reps)
    stem.input_grad = False
    print('stem backward, [%d, 3, 32, 32], 256 filters (median of %d, ms):' % (batch, reps))
    for k, v in res.items():
        print('  %-46s %8.3f' % (k, v))
    return res


def conv0_dgrad(batch, reps):
    from torch.profiler import ProfilerActivity, profile
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    shape = _lib.NodeStemShape(batch, 3, 32, 32, 64, 1e-5)
    nbytes = lib.node_stem_conv0_dgrad_workspace_bytes(C.byref(shape))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    w0 = torch.randn(64, 3, 3, 3, device='cuda')
    dy = torch.randn(batch, 64, 30, 30, device='cuda')
    dx = torch.empty(batch, 3, 32, 32, device='cuda')

    def call():
        _lib.check(lib.node_stem_conv0_dgrad(C.byref(shape), w0.data_ptr(), dy.data_ptr(), dx.data_ptr(), (ws.data_ptr() + 255) & ~255,
                                             nbytes, torch.cuda.current_stream().cuda_stream))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
    moved = dy.numel() * 4 + dx.numel() * 4
    us = None
    for e in prof.key_averages():
        if 'k_stem_conv0_dgrad' in e.key:
            total = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0)
            us = total / max(e.count, 1)
    print('k_stem_conv0_dgrad alone, [%d, 3, 32, 32]: dh0 %.1f MB + image %.1f MB' % (batch, dy.numel() * 4 / 1e6, dx.numel() * 4 / 1e6))
    if us:
        print('  %.1f us per launch (profiler kernel records, %d launches): %.0f GB/s of the bytes it must move' % (us, reps, moved / us / 1e3))
    else:
        whole = _alternate({'entry': (None, call)}, reps)['entry']
        print('  no kernel record from the profiler; the diagnostics entry (NCHW -> NHWC transposition + kernel): %.3f ms' % whole)
    return us


def attack_iteration(batch, reps, iterations=3):
    import neural_ode_features_amd as nof
    from neural_ode_features_amd.attack import bim, bim_reference
    torch.manual_seed(0)
    net = nof.ODENet(3, out=10, n_filters=256, downsample='residual', adjoint=True, method='dopri5', tol=1e-3).cuda().eval()
    x = torch.rand(batch, 3, 32, 32, device='cuda')
    with torch.no_grad():
        mean = torch.tensor(CIFAR[0], device='cuda').reshape(1, 3, 1, 1)
        std = torch.tensor(CIFAR[1], device='cuda').reshape(1, 3, 1, 1)
        y = net((x - mean) / std).argmax(1)
    kw = dict(norm=2, epsilon=.05, stepsize=.02, iterations=iterations, return_early=False, preprocessing=CIFAR)

    def frozen(flag):
        for p in net.parameters():
            p.requires_grad_(not flag)
    variants = {
        'library path, fused stem': (None, lambda: bim(net, x, y, **kw)),
        'library path, module-sequence stem': (None, lambda: bim(net, x, y, fused_stem=False, **kw)),
        'plain-torch loop, default path': (None, lambda: bim_reference(net, x, y, **kw)),
        'plain-torch loop, default path, frozen parameters': (lambda: frozen(True), lambda: (bim_reference(net, x, y, **kw), frozen(False))),
    }
    res = _alternate(variants, max(3, reps // 4), warm=2)
    print('one attack iteration (L2, dopri5 tol 1e-3, 256 filters), [%d, 3, 32, 32]: ms per iteration = whole attack / %d' % (batch, iterations))
    for k, v in res.items():
        print('  %-52s %9.3f' % (k, v / iterations))
    return res


def dopri5_gradient():
    from tests import test_gpu_attack as T
    net = T._net(0, method='dopri5')
    oracle32 = T.RefODENet(net, torch.float32)
    x = T._images(0)
    net = net.cuda()
    with torch.no_grad():
        labels = net(T._normalise(x.cuda(), CIFAR)).argmax(1)
    def steps():
        f = net.odeblock.odefunc
        fs, bs = getattr(f, 'last_forward_stats', None) or {}, getattr(f, 'last_backward_stats', None) or {}
        return 'forward %s+%s, adjoint %s+%s' % (fs.get('accepted'), fs.get('rejected'), bs.get('accepted'), bs.get('rejected'))
    g_mod, _ = T._input_gradient(net, x.cuda(), labels, CIFAR, fused=False)
    steps_mod = steps()
    g_fused, _ = T._input_gradient(net, x.cuda(), labels, CIFAR, fused=True)
    steps_fused = steps()
    with torch.no_grad():      # how far apart the two stems' outputs are: what the two solves start from
        stem = net.downsample.module
        xin = T._normalise(x.cuda(), CIFAR)
        h_fused = stem(xin)
        h_mod = torch.nn.Sequential.forward(stem, xin)
    print('  stem output, fused against module sequence: %.3e of max|h|' % float((h_fused - h_mod).abs().max() / h_mod.abs().max()))
    print('  accepted+rejected steps: default path %s; fused-stem path %s' % (steps_mod, steps_fused))
    g_cpu, _ = T._input_gradient(oracle32, x, labels.cpu(), CIFAR)
    d_default = float((g_mod.cpu() - g_cpu).abs().max() / g_cpu.abs().max())
    d_fused = float((g_fused - g_mod).abs().max() / g_mod.abs().max())
    print('dopri5 input gradient, ODENet(3, 64 filters, residual), [4, 3, 32, 32], tol 1e-3, max |difference| / max |reference|:')
    print('  default path (module-sequence stem) against the oracle\'s fp32 CPU run   %.3e' % d_default)
    print('  fused-stem path against the default path on the device                 %.3e' % d_fused)
    return d_default, d_fused


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[128, 1])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', choices=('stem', 'kernel', 'iteration', 'dopri5'), nargs='+', default=None)
    args = ap.parse_args(argv)
    want = set(args.only or ('stem', 'kernel', 'iteration', 'dopri5'))
    print('device:', torch.cuda.get_device_name(0))
    for b in args.batches:
        if 'stem' in want:
            stem_backward(b, args.reps)
        if 'kernel' in want:
            conv0_dgrad(b, args.reps)
        if 'iteration' in want:
            attack_iteration(b, args.reps)
    if 'dopri5' in want:
        dopri5_gradient()


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Times of the image convolution in front of the ODE block (imgconv.py, csrc/kernels_imgconv.hip) against the path it replaces
-- the same module with `nn.Conv2d.forward` called directly (MIOpen / ATen) -- in ONE process, alternating the two:

    hipcc --offload-arch=gfx950 -O3 tools/hbm_stream.hip -o tools/hbm_stream
    python3 tools/imgconv_time.py > profiles/imgconv_time.txt

Per shape: forward, backward without d_x, backward with d_x, each as HIP events around a run of `--reps` calls of the module / of
torch.autograd.grad from Python (what a training step sees: dispatch included), alternating the two paths round by round, median
over the rounds.  `fused, C ABI` is the library's entry points called back to back on preallocated buffers (the kernels' own time).
The large operand of every call -- grad_y of the backwards, y of the C ABI forward -- ROTATES through enough buffers to exceed the
256 MB Infinity Cache between two uses of one of them, so the times are cache-cold like the copy rate next to them; the module
forward's y comes from the caching allocator (the same block call after call: its writes may stay in that cache), for both paths
alike.  Next to the times: what ONE pass over y takes at the copy rate tools/hbm_stream reports on this box (its best cold rate,
run as a child process before this one opens the GPU), and the worst |error| / bound of the fused results against fp64 (bound:
2 (t + 2) 2^-24 A, tests/test_gpu_imgconv.py)."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 3, 32, 32, 256), (128, 1, 28, 28, 64)]


def copy_rate():
    """TB/s: the best cold (rotating buffers) line of tools/hbm_stream."""
    exe = os.path.join(ROOT, 'tools', 'hbm_stream')
    if not os.path.exists(exe):
        subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', exe + '.hip', '-o', exe])
    out = subprocess.check_output([exe], text=True, timeout=300)
    rates = [float(m.group(1)) for line in out.splitlines() if line.startswith('cold') for m in [re.search(r'([\d.]+) TB/s', line)] if m]
    return max(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--copy-rate', type=float, default=None, help='TB/s; default: run tools/hbm_stream')
    ap.add_argument('--reps', type=int, default=400)
    ap.add_argument('--rounds', type=int, default=9)
    a = ap.parse_args()
    rate = a.copy_rate if a.copy_rate else copy_rate()

    import torch
    import torch.nn.functional as F
    from torch import nn
    import neural_ode_features_amd as nof
    assert torch.cuda.is_available(), 'needs a HIP device'
    print('device: %s; copy rate %.2f TB/s (tools/hbm_stream, cold)' % (torch.cuda.get_device_name(0), rate))

    def eager(setup):
        fn = setup()
        for _ in range(10):
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

    def abi(call):
        """The library's entry points called back to back on preallocated buffers: no autograd, no allocation, launches queue up
        behind each other -- the kernels' own time."""
        return eager(lambda: call)

    for shape in SHAPES:
        n, cin, h, w, filters = shape
        torch.manual_seed(0)
        m = nof.ImageConv2d(cin, filters).cuda()
        x = torch.randn(n, cin, h, w, device='cuda')
        xg = x.clone().requires_grad_(True)
        dy = torch.randn(n, filters, h // 2, w // 2, device='cuda')
        ybytes = dy.numel() * 4
        nsets = min(64, max(2, -(-320 * 1000 * 1000 // ybytes)))       # 320 MB of grad_y between two uses of one buffer
        dys = [dy] + [torch.randn_like(dy) for _ in range(nsets - 1)]

        def rotating(fns):
            i = [0]

            def fn():
                i[0] = (i[0] + 1) % len(fns)
                return fns[i[0]]()
            return fn
        paths = {'fused': lambda t: m(t), 'parent': lambda t: nn.Conv2d.forward(m, t)}
        params = [m.weight, m.bias]
        work = {}
        def backward_of(fwd, inp, wrt):
            def setup():
                ys = [fwd(inp) for _ in dys]
                return rotating([lambda y=y, d=d: torch.autograd.grad(y, wrt, d, retain_graph=True) for y, d in zip(ys, dys)])
            return setup
        for name, fwd in paths.items():
            work[name] = {
                'forward': (lambda fwd=fwd: (lambda: fwd(x))),
                'backward': backward_of(fwd, x, params),
                'backward + d_x': backward_of(fwd, xg, params + [xg]),
            }
        # accuracy of the fused results against fp64
        y = m(xg)
        dw, db, dx = torch.autograd.grad(y, params + [xg], dy)
        got = {'y': y.detach(), 'dw': dw, 'db': db, 'dx': dx}

        def fp64(xx, ww, bb, dd):
            xx, ww, bb = [t.detach().double().cpu().requires_grad_(True) for t in (xx, ww, bb)]
            yy = F.conv2d(xx, ww, bb, 2, 1)
            gx, gw, gb = torch.autograd.grad(yy, (xx, ww, bb), dd.detach().double().cpu())
            return {'y': yy.detach(), 'dw': gw, 'db': gb, 'dx': gx}
        ref, mag = fp64(x, m.weight, m.bias, dy), fp64(x.abs(), m.weight.abs(), m.bias.abs(), dy.abs())
        red = n * (h // 2) * (w // 2)
        terms = {'y': 16 * cin, 'dw': red, 'db': red, 'dx': 4 * filters}
        ratio = max(float(((got[k].double().cpu() - ref[k]).abs() / (2.0 * (t + 2) * 2.0 ** -24 * mag[k])).max()) for k, t in terms.items())

        print('\nx [%d, %d, %d, %d] -> %d filters: y is %.1f MB, one pass over y at the copy rate %.1f us; fused max |err| / bound %.3f'
              % (n, cin, h, w, filters, ybytes / 1e6, ybytes / rate / 1e6, ratio))
        print('%d calls per timed window, the large operand rotating through %d buffers (%.0f MB)' % (a.reps, nsets, nsets * ybytes / 1e6))
        from neural_ode_features_amd import _lib
        import ctypes as C
        lib = _lib.load()
        sh = _lib.NodeImgConvShape(*shape)
        nbytes = lib.node_imgconv_workspace_bytes(C.byref(sh))
        ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        ybs = [torch.empty_like(dy) for _ in dys]
        dwb, dbb, dxb = torch.empty_like(m.weight), torch.empty_like(m.bias), torch.empty_like(x)
        wt, bs = m.weight.detach(), m.bias.detach()
        stream = torch.cuda.current_stream().cuda_stream

        def bwd_call(dx_ptr):
            return rotating([lambda d=d.data_ptr(): _lib.check(lib.node_imgconv_bwd(
                C.byref(sh), x.data_ptr(), wt.data_ptr(), d, dwb.data_ptr(), dbb.data_ptr(), dx_ptr, ws.data_ptr(), nbytes, stream))
                for d in dys])
        calls = {
            'forward': rotating([lambda yb=yb.data_ptr(): _lib.check(lib.node_imgconv_fwd(
                C.byref(sh), x.data_ptr(), wt.data_ptr(), bs.data_ptr(), yb, stream)) for yb in ybs]),
            'backward': bwd_call(None),
            'backward + d_x': bwd_call(dxb.data_ptr()),
        }
        print('%-16s %12s %12s %16s' % ('', 'fused us', 'parent us', 'fused, C ABI us'))
        totals = {}
        for what in ('forward', 'backward', 'backward + d_x'):
            runs = {p: eager(work[p][what]) for p in paths}
            runs['abi'] = abi(calls[what])
            t = {p: [] for p in runs}
            for _ in range(a.rounds):                      # alternate the paths round by round
                for p in runs:
                    t[p].append(runs[p]())
            med = {p: statistics.median(v) for p, v in t.items()}
            totals[what] = med
            print('%-16s %12.1f %12.1f %16.1f     (min %.1f / %.1f / %.1f)'
                  % (what, med['fused'], med['parent'], med['abi'], min(t['fused']), min(t['parent']), min(t['abi'])))
        f = totals['forward']['fused'] + totals['backward']['fused']
        p = totals['forward']['parent'] + totals['backward']['parent']
        print('forward + backward (no d_x): fused %.1f us, parent %.1f us, parent / fused %.2f' % (f, p, p / f))


if __name__ == '__main__':
    main()

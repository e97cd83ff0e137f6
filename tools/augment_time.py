#!/usr/bin/env python
"""Cost of the device input pipeline (augment.py, csrc/kernels_augment.hip) at the CIFAR batch -- 128 images of 3 x 32 x 32,
all stages (`crop+jitter+flip+norm`) -- and what it does to the training step.

    python3 tools/augment_time.py launch                 # HIP events around Augmenter.batch
    rocprofv3 --kernel-trace --stats -d /tmp/at -o at -- python3 tools/augment_time.py launch --iters 200
    python3 tools/augment_time.py report /tmp/at         # k_augment durations from that trace, bytes moved over time
    python3 tools/augment_time.py step                   # wall time per training step, same process, alternating:
                                                         #   host   the loop without the flag: fp32 images on the host, gathered
                                                         #          there, one pageable host-to-device copy per batch
                                                         #   device --augmentation crop+flip+norm: one launch per batch
The step measurement trains the CIFAR-10 configuration (`-d residual -f 256 -a`, batch 128, deferred completion) with a
learning rate of zero, so that every pass does the same solver work; `host` gets the device pipeline's test transform of the
same 8-bit images as fp32 (the same numbers the parent's loop would be fed).
"""
import argparse
import csv
import glob
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCH, SHAPE = 128, (3, 32, 32)
BYTES = BATCH * (3 * 32 * 32 * (1 + 4) + 8 + 8 + 8)         # uint8 pixels in, fp32 out, index + label in, label out


def _split(n, seed=0):
    import torch
    import neural_ode_features_amd as nof
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n,) + SHAPE, generator=gen, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=gen)
    return nof.DeviceSplit(x, y, 'cuda'), x, y


def launch(iters, warmup):
    import torch
    import neural_ode_features_amd as nof
    split, _, _ = _split(50000)
    aug = nof.Augmenter('crop+jitter+flip+norm', dataset='cifar10', seed=23)
    perm = torch.randperm(len(split), generator=torch.Generator().manual_seed(1)).cuda()
    for i in range(warmup):
        aug.batch(split, perm[i * BATCH:(i + 1) * BATCH], 1)
    torch.cuda.synchronize()
    times = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        j = (i % (len(split) // BATCH)) * BATCH
        a.record()
        aug.batch(split, perm[j:j + BATCH], 1)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    t = np.array(times)
    print('Augmenter.batch, %d x %s, crop+jitter+flip+norm, HIP events around the call (allocation + launch): median %.1f us  '
          'min %.1f  max %.1f  (%d calls)' % (BATCH, 'x'.join(map(str, SHAPE)), np.median(t), t.min(), t.max(), iters), flush=True)


def report(dirname):
    files = glob.glob(os.path.join(dirname, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel trace under %s' % dirname)
    d = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in csv.DictReader(open(files[0]))
         if 'k_augment' in r['Kernel_Name']]
    if not d:
        raise SystemExit('no k_augment launch in %s' % files[0])
    d = np.array(d[len(d) // 10:])                          # the first tenth: warm-up
    print('k_augment<3>, %d x %s, all stages, rocprofv3 kernel durations: launches %d  median %.2f us  min %.2f  max %.2f;  '
          '%.2f MB moved per launch -> %.0f GB/s at the median'
          % (BATCH, 'x'.join(map(str, SHAPE)), len(d), np.median(d), d.min(), d.max(), BYTES / 1e6, BYTES / np.median(d) / 1e3))


def step(steps, passes, filters):
    import torch
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import train as T
    args = types.SimpleNamespace(batch_size=BATCH, batch_accumulation=1, adjoint=True, method='dopri5', device=torch.device('cuda'))
    split, x, y = _split(steps * BATCH)
    aug = nof.Augmenter('crop+flip+norm', dataset='cifar10', seed=23)
    order = torch.arange(len(split), device='cuda')
    host_x = torch.cat([aug.batch(split, order[i:i + 1024], 0, train=False)[0] for i in range(0, len(split), 1024)]).cpu()
    torch.manual_seed(0)
    model = nof.ODENet(3, out=10, n_filters=filters, downsample='residual', method='dopri5', tol=1e-3, adjoint=True).cuda()
    opt = nof.FusedSGD(model.parameters(), lr=0.0, momentum=0.9, weight_decay=0.0)
    loop = T.deferred_loop(model, opt, args)
    feeds = {'host': (host_x, y), 'device': (split, aug)}
    per = {k: [] for k in feeds}
    for p in range(passes + 1):                              # pass 0 of each: warm-up
        for name, data in feeds.items():
            gen = torch.Generator().manual_seed(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = T.train(data, model, opt, args, gen, loop, epoch=1)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps * 1e3
            if p:
                per[name].append(dt)
            print('pass %d %-6s %.3f ms per step (%d steps of %d; nfe-f %.1f nfe-b %.1f)%s'
                  % (p, name, dt, steps, BATCH, m['nfe-f'], m['nfe-b'], '  [warm-up]' if not p else ''), flush=True)
    for name, v in per.items():
        print('%-6s median %.3f ms per step  min %.3f  max %.3f  -> %.0f images/s' % (name, np.median(v), min(v), max(v),
                                                                                    BATCH / np.median(v) * 1e3))
    print('device / host = %.3f' % (np.median(per['device']) / np.median(per['host'])))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('launch', 'report', 'step'))
    ap.add_argument('dir', nargs='?', default=None)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--filters', type=int, default=256)
    a = ap.parse_args()
    if a.mode == 'report':
        report(a.dir)
    elif a.mode == 'launch':
        launch(a.iters, a.warmup)
    else:
        step(a.steps, a.passes, a.filters)

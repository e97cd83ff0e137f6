#!/usr/bin/env python
"""Time of one retrieval evaluation call (`retrieval.average_precision`, Nq = Nd = 10 000, the CIFAR-10 test split against
itself) at D = 64 and 256, by HIP events; the reference's host path (one sklearn average_precision_score per query, plus the
argsort of AP@10, evaluate.py:336-346) on a 500-query subset of the same data, on the host cores.

    python3 tools/retrieval_time.py                      # events + sklearn
    rocprofv3 --kernel-trace --stats -d /tmp/rt -o rt -- python3 tools/retrieval_time.py --gpu-only --iters 5
    python3 tools/retrieval_time.py --report /tmp/rt     # scoring vs ranking kernel time from that trace
"""
import argparse
import csv
import glob
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 10000


def data(d, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((N, d)).astype(np.float32)
    f /= np.linalg.norm(f, axis=-2, keepdims=True) + 1e-7          # as evaluate.py:326 normalises
    return f, rng.integers(0, 10, N).astype(np.int32)


def gpu(d, iters, warmup):
    import torch
    from neural_ode_features_amd.retrieval import average_precision
    f, y = data(d)
    fd, yd = torch.from_numpy(f).cuda(), torch.from_numpy(y).cuda()
    for _ in range(warmup):
        average_precision(fd, fd, yd, yd, k=10)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        average_precision(fd, fd, yd, yd, k=10)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times = np.array(times)
    print('GPU  D=%-4d Nq=Nd=%d  average_precision (AP + AP@10): median %.3f ms  min %.3f  max %.3f  (%d calls)'
          % (d, N, np.median(times), times.min(), times.max(), iters), flush=True)
    return float(np.median(times))


def host(d, nq):
    from sklearn.metrics import average_precision_score
    f, y = data(d)
    gt = y[:nq, None] == y[None, :]
    t0 = time.perf_counter()
    s = f[:nq].dot(f.T)
    t1 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in range(nq):
            average_precision_score(gt[i], s[i])
        t2 = time.perf_counter()
        ranking = s.argsort(axis=1)[:, ::-1][:, :10]
        rows = np.arange(nq)[:, None]
        rs, rg = s[rows, ranking], gt[rows, ranking]
        for i in range(nq):
            average_precision_score(rg[i], rs[i])
    t3 = time.perf_counter()
    cores = len(os.sched_getaffinity(0))
    per_q = (t3 - t0) / nq
    print('host D=%-4d %d queries x %d items on %d cores: scores %.1f ms, AP %.1f ms, AP@10 (argsort + sklearn) %.1f ms; '
          '%.2f ms per query -> %.1f s for %d queries (one asym or sym pass of AP + AP@10)'
          % (d, nq, N, cores, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * per_q, per_q * N, N), flush=True)


def report(dirname):
    files = glob.glob(os.path.join(dirname, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel trace under %s' % dirname)
    per = {}
    for r in csv.DictReader(open(files[0])):
        name = r['Kernel_Name']
        stage = 'scoring (k_ret_scores)' if 'k_ret_scores' in name else 'ranking (k_ret_rank)' if 'k_ret_rank' in name else None
        if stage:
            per.setdefault(stage, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6)
    for k, v in sorted(per.items()):
        print('%-20s launches %4d  total %9.3f ms  mean %.3f ms' % (k, len(v), sum(v), sum(v) / len(v)))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--dims', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-queries', type=int, default=500)
    ap.add_argument('--gpu-only', action='store_true')
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--report', default=None)
    a = ap.parse_args()
    if a.report:
        report(a.report)
        sys.exit(0)
    for d in a.dims:
        if not a.host_only:
            gpu(d, a.iters, a.warmup)
        if not a.gpu_only:
            host(d, a.host_queries)

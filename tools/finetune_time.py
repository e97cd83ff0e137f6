#!/usr/bin/env python
"""Time of the finetune evaluation's grid search on ONE slice of features [10000, 256], 10 classes (the CIFAR-10 test split,
`finetune.linear_svc_cv`: 5 folds + refit, 5 Cs, 10 classes = 300 problems), end to end by wall clock around a synchronised
call, and the host path of the reference, `GridSearchCV(LinearSVC(dual=False), n_jobs=16)`, on the same features and the
same machine.  The Hessian-vector launch alone comes from a kernel trace.  Writes profiles/finetune_time.txt.

    python3 tools/finetune_time.py                       # GPU end to end + sklearn
    rocprofv3 --kernel-trace --output-format csv -d /tmp/ft -o ft -- python3 tools/finetune_time.py --gpu-only --iters 1
    python3 tools/finetune_time.py --report /tmp/ft      # per-kernel times of that trace, the Hv launch against its bounds

The features follow tests/golden/make_golden_finetune.py: max(mu[y] + N(0, 1), 0) * 0.25, sep 0.12.
"""
import argparse
import csv
import glob
import os
import platform
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, K, P = 10000, 256, 10, 300
HBM_TBS, MFMA_F32_TF = 6.3, 155.0          # achievable HBM bandwidth and fp32 matrix rate of an MI355X


def data(seed=0, sep=0.12):
    rng = np.random.default_rng(seed)
    y = rng.permutation(np.arange(N) % K).astype(np.int64)
    mu = sep * rng.standard_normal((K, D))
    return (np.maximum(mu[y] + rng.standard_normal((N, D)), 0.0) * 0.25).astype(np.float32), y


def gpu(iters, warmup, out):
    import torch
    from neural_ode_features_amd.finetune import linear_svc_cv
    x, y = data()
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    times, res = [], None
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = linear_svc_cv(xd, yd)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    times = np.array(times)
    out('GPU  %s: linear_svc_cv [%d, %d], %d classes, %d problems: median %.1f ms  min %.1f  max %.1f  (%d calls); '
        'Newton iterations <= %d, converged %d / %d, best C %g, cv accuracy %.4f'
        % (torch.cuda.get_device_name(0), N, D, K, P, np.median(times), times.min(), times.max(), iters, res.n_iter.max(),
           res.converged.sum(), len(res.converged), res.best_C, res.best_score))
    return res


def host(jobs, out):
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import LinearSVC
    x, y = data()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        t0 = time.perf_counter()
        gs = GridSearchCV(LinearSVC(dual=False), {'C': np.logspace(-2, 2, 5)}, scoring='accuracy', cv=5, n_jobs=jobs).fit(x, y)
        t1 = time.perf_counter()
    out('host %s, %d of %d cores: GridSearchCV(LinearSVC(dual=False), n_jobs=%d) on the same features: %.1f s; best C %g, cv '
        'accuracy %.4f' % (platform.processor() or platform.machine(), jobs, len(os.sched_getaffinity(0)), jobs, t1 - t0,
                           gs.best_params_['C'], gs.best_score_))


def report(dirname, out):
    files = glob.glob(os.path.join(dirname, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel trace under %s' % dirname)
    per = {}
    for r in csv.DictReader(open(files[0])):
        name = r['Kernel_Name']
        if 'k_svm_' not in name:
            continue
        key = name[name.index('k_svm_'):].split('(')[0]
        per.setdefault(key, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    for k, v in sorted(per.items()):
        v = np.array(v)
        out('%-28s launches %5d  total %10.1f us  median %8.1f  max %8.1f' % (k, len(v), v.sum(), np.median(v), v.max()))
    hv = np.array([t for k, v in per.items() if k.startswith('k_svm_product<1>') or k.startswith('k_svm_product<(int)1>') for t in v])
    if len(hv):
        full = hv[hv >= 0.8 * hv.max()]          # launches with every problem tile still open (a finished tile exits at once)
        d1 = D + 1
        byts = 4.0 * (N * D + 2 * P * d1)
        flops = 4.0 * N * d1 * P
        t_hbm, t_mfma = byts / (HBM_TBS * 1e12) * 1e6, flops / (MFMA_F32_TF * 1e12) * 1e6
        t = float(np.median(full))
        out('Hessian-vector launch, all %d problems open: median %.1f us over %d launches; it must move %.2f MB (X once, V and Hv '
            'once): %.1f us at %.1f TB/s; %.2f GFLOP on the fp32 matrix pipe: %.1f us at %.0f TF -> the fp32 MFMA rate binds, the '
            'launch runs at %.0f %% of it' % (P, t, len(full), byts / 1e6, t_hbm, HBM_TBS, flops / 1e9, t_mfma, MFMA_F32_TF,
                                             100.0 * t_mfma / t))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--jobs', type=int, default=16)
    ap.add_argument('--gpu-only', action='store_true')
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--report', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'finetune_time.txt'))
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if a.report:
        report(a.report, out)
    else:
        if not a.host_only:
            gpu(a.iters, a.warmup, out)
        if not a.gpu_only:
            host(a.jobs, out)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')

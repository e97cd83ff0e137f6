#!/usr/bin/env python
"""Generate the fixtures of the finetune evaluation (finetune.py, csrc/kernels_svm.hip) under tests/golden/ with sklearn,
on the CPU:

    python tests/golden/make_golden_finetune.py

What the reference's `evaluate.py finetune` runs per time slice is `GridSearchCV(LinearSVC(), C = logspace(-2, 2, 5), cv=5)`:
one-vs-rest squared-hinge problems with a regularised bias,

    f(w~) = 1/2 |w~|^2 + C sum_i max(0, 1 - y_i w~ . [x_i, 1])^2      over the rows of the training folds.

f is strictly convex, so the fixtures store its fp64 minimiser and everything is compared against that.

  finetune_small.npz   N = 603, D = 33,  K = 10, the five Cs     unequal folds, D + 1 = 34 is no multiple of a tile, P = 300
  finetune_tiny.npz    N = 157, D = 7,   K = 3,  the five Cs     fewer rows and columns than one tile
  finetune_pair.npz    N = 90,  D = 5,   K = 2,  Cs 0.1, 1, 10   the one-problem binary path
  finetune_wide.npz    N = 1030, D = 256, K = 10, Cs 0.01, 0.1, 1  the real feature width; X is stored as uint8 x scale

Features are max(mu[y] + N(0, 1), 0) * 0.25 with mu = sep * N(0, 1) per class: non-negative, like pooled ReLU features.
Labels are a permutation of arange(N) % K.

Each file holds
  X (or Xq uint8 and scale), labels, fold_ids                     fold ids of sklearn's StratifiedKFold(5), no shuffling
  Cs, classes
  prob_fold, prob_class, prob_C  [P]                              the problem table: folds 0..4 and -1 (the refit on all
                                                                  rows), times Cs, times classes (two classes: classes[1] only)
  w_star [P, D + 1], f_star [P]                                   fp64 optimum: LinearSVC(dual=False, tol=1e-12,
                                                                  max_iter=100000) on float64 features, then polished by
                                                                  exact fp64 Newton steps until f stops decreasing
  grad_star [P]                                                   |grad f(w*)| / |grad f(0)|: how converged the optimum is
  z_star [|Cs|, K', N]                                            w*(fold of row i, C, class) . [x_i, 1]: held-out decisions
  dz_ref, gap_ref [|Cs|]                                          the reference as run, LinearSVC(C, dual=False) with its
                                                                  default tol on the float32 features, per fold and class:
                                                                  max |z_ref - z*| on held-out rows, max (f(w_ref) - f*) / f*
  knife [|Cs|, N] bool                                            held-out samples whose fp64 top-two margin is below
                                                                  4 dz_ref(C) (two classes: |z*| below it)
  mean_test_score [|Cs|], best_score                              GridSearchCV(LinearSVC(dual=False), cv=5)

The generator asserts that the knife-edge share stays at or below 5 % in every (fold, C) (for the wide fixture after the
uint8 quantisation); where a fixture misses the cap it shrinks `sep` until the cap is met (never the cap).  The more
separable the classes, the worse conditioned the problems at C = 100 and the further the reference's own solver strays.
"""
import os
import warnings

import numpy as np
from sklearn.model_selection import GridSearchCV, StratifiedKFold
from sklearn.svm import LinearSVC

HERE = os.path.dirname(os.path.abspath(__file__))
KNIFE_CAP = 0.05
ALL_CS = np.logspace(-2, 2, 5)


def make_data(n, d, k, sep, seed):
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.arange(n) % k).astype(np.int64)
    mu = sep * rng.standard_normal((k, d))
    x = np.maximum(mu[labels] + rng.standard_normal((n, d)), 0.0) * 0.25
    return x.astype(np.float32), labels


def objective(w, xt, y, c):
    h = np.maximum(0.0, 1.0 - y * (xt @ w))
    return 0.5 * w @ w + c * (h @ h)


def gradient(w, xt, y, c):
    z = xt @ w
    a = (1.0 - y * z) > 0
    return w + 2.0 * c * (xt[a].T @ (z[a] - y[a]))


def polish(w, xt, y, c, steps=50):
    """Exact fp64 Newton steps from liblinear's answer, kept while f decreases."""
    f = objective(w, xt, y, c)
    for _ in range(steps):
        z = xt @ w
        a = (1.0 - y * z) > 0
        g = w + 2.0 * c * (xt[a].T @ (z[a] - y[a]))
        h = np.eye(len(w)) + 2.0 * c * (xt[a].T @ xt[a])
        w2 = w - np.linalg.solve(h, g)
        f2 = objective(w2, xt, y, c)
        if not f2 < f:
            break
        w, f = w2, f2
    return w, f


def reference_solution(x, labels, cs):
    """Everything the tests compare against, for float32 features `x [N, D]`: the fold ids, the problem table, the fp64
    optimum of every problem, the reference solver's own distance from it and the knife-edge set (see the module docstring).
    Returns (dict of arrays, largest knife-edge share over the (fold, C))."""
    n, d = x.shape
    classes = np.unique(labels)
    fold_ids = np.empty(n, np.int32)
    for f, (_, test) in enumerate(StratifiedKFold(5).split(x, labels)):
        fold_ids[test] = f
    x64 = x.astype(np.float64)
    xt = np.concatenate([x64, np.ones((n, 1))], 1)
    targets = classes[1:] if len(classes) == 2 else classes
    kk = len(targets)
    pf, pc, pcs, w_star, f_star, g_star = [], [], [], [], [], []
    z_star = np.zeros((len(cs), kk, n))
    dz_ref = np.zeros(len(cs))
    gap_ref = np.zeros(len(cs))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for fold in list(range(5)) + [-1]:
            train = fold_ids != fold
            held = ~train
            for ci, c in enumerate(cs):
                for ki, cls in enumerate(targets):
                    y = np.where(labels == cls, 1.0, -1.0)
                    svc = LinearSVC(C=c, dual=False, tol=1e-12, max_iter=100000).fit(x64[train], y[train])
                    w = np.concatenate([svc.coef_[0], svc.intercept_])
                    w, f = polish(w, xt[train], y[train], c)
                    pf.append(fold), pc.append(cls), pcs.append(c), w_star.append(w), f_star.append(f)
                    g0 = np.linalg.norm(gradient(np.zeros(d + 1), xt[train], y[train], c))
                    g_star.append(np.linalg.norm(gradient(w, xt[train], y[train], c)) / g0)
                    if fold < 0:
                        continue
                    z_star[ci, ki, held] = xt[held] @ w
                    ref = LinearSVC(C=c, dual=False).fit(x[train], y[train])      # the reference as run: float32 features
                    wr = np.concatenate([ref.coef_[0], ref.intercept_]).astype(np.float64)
                    dz_ref[ci] = max(dz_ref[ci], np.abs(xt[held] @ wr - xt[held] @ w).max())
                    gap_ref[ci] = max(gap_ref[ci], (objective(wr, xt[train], y[train], c) - f) / f)
        gs = GridSearchCV(LinearSVC(dual=False), {'C': cs}, scoring='accuracy', cv=5).fit(x, labels)
    knife = np.zeros((len(cs), n), bool)
    worst = 0.0
    for ci in range(len(cs)):
        if kk == 1:
            margin = np.abs(z_star[ci, 0])
        else:
            top = np.sort(z_star[ci], axis=0)
            margin = top[-1] - top[-2]
        knife[ci] = margin < 4.0 * dz_ref[ci]
        for f in range(5):
            worst = max(worst, knife[ci][fold_ids == f].mean())
    out = dict(labels=labels, fold_ids=fold_ids, Cs=np.asarray(cs, np.float64), classes=classes,
               prob_fold=np.array(pf, np.int32), prob_class=np.array(pc, np.int64), prob_C=np.array(pcs, np.float64),
               w_star=np.array(w_star), f_star=np.array(f_star), grad_star=np.array(g_star), z_star=z_star, dz_ref=dz_ref,
               gap_ref=gap_ref, knife=knife, mean_test_score=gs.cv_results_['mean_test_score'], best_score=gs.best_score_)
    return out, worst


def fixture(name, n, d, k, cs, sep, seed, quantise=False):
    x, labels = make_data(n, d, k, sep, seed)
    if quantise:
        scale = np.float32(x.max() / 255.0)
        xq = np.clip(np.rint(x / scale), 0, 255).astype(np.uint8)
        x = xq.astype(np.float32) * scale
        extra = {'Xq': xq, 'scale': scale}
    else:
        extra = {'X': x}
    out, worst = reference_solution(x, labels, cs)
    out.update(extra, sep=sep, seed=seed)
    print('%-6s sep %.3f  dz_ref %s  gap_ref %s  knife-edge share max %.4f  grad* max %.1e  best %.4f'
          % (name, sep, np.array2string(out['dz_ref'], precision=2), np.array2string(out['gap_ref'], precision=2), worst,
             out['grad_star'].max(), out['best_score']), flush=True)
    return out, worst


def write(name, out):
    path = os.path.join(HERE, 'finetune_%s.npz' % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, (path, size)
    print('  ->', path, size, 'bytes', flush=True)


def main():
    # (name, N, D, K, Cs, first sep, seed, quantise): `sep` shrinks by 0.8 until the knife-edge cap is met; the cap never moves
    for name, n, d, k, cs, sep, seed, quantise in (('small', 603, 33, 10, ALL_CS, 0.35, 1, False),
                                                   ('tiny', 157, 7, 3, ALL_CS, 0.8, 2, False),
                                                   ('pair', 90, 5, 2, np.array([0.1, 1.0, 10.0]), 0.8, 3, False),
                                                   ('wide', 1030, 256, 10, np.array([0.01, 0.1, 1.0]), 0.12, 4, True)):
        for _ in range(8):
            out, worst = fixture(name, n, d, k, cs, sep, seed, quantise=quantise)
            if worst <= KNIFE_CAP:
                break
            sep *= 0.8
        assert worst <= KNIFE_CAP, (name, worst)
        write(name, out)


if __name__ == '__main__':
    main()

"""Finetune evaluation on the HIP backend: the cross-validated linear SVM of `evaluate.py finetune` in the reference
(evaluate.py:364-413), which runs `GridSearchCV(LinearSVC(), {'C': logspace(-2, 2, 5)}, cv=5, scoring='accuracy')` on the host
for every time slice of the extracted features.

    search = linear_svc_cv(x, labels)                   # x [N, D] float32 on the device, integer labels [N]
    search.best_score, search.best_C, search.coef, search.intercept

`LinearSVC()` is one squared-hinge, L2-regularised problem per class (one-vs-rest) with a regularised bias,

    f(w~) = 1/2 |w~|^2 + C sum_i max(0, 1 - y_i w~ . [x_i, 1])^2      over the rows of the training folds,

so a grid search is (folds + 1 refit) x |Cs| x K problems over ONE feature matrix that differ only in a row mask, a target
sign and C.  `linear_svc_fit` solves them all at once by a truncated Newton method whose products run on the fp32 matrix pipe
(csrc/kernels_svm.hip); f is strictly convex, so the result is its unique minimiser, whichever solver finds it.  A problem
stops at liblinear's rule |grad f(w)| <= eps max(min(#pos, #neg), 1) / n |grad f(0)|.  DEFAULT_EPS = 1e-5 is a tenth of
LinearSVC's default `tol`: the fp32 solver is then no further from the fp64 optimum than twice the distance at which
liblinear's own primal solver stops at its default (tests/test_gpu_finetune.py, profiles/finetune_parity.txt).  A problem that
does not get there within `max_iter` Newton iterations is reported in `converged` and warned about.

Folds are sklearn's `StratifiedKFold(folds)` without shuffling; scores are per-fold accuracies, their unweighted mean per C,
and the first maximum among the Cs.  Results are bit-identical from run to run.  There is no CPU path.
"""
from __future__ import annotations

import types
import warnings

import numpy as np
import torch

from . import _lib, workspace

DEFAULT_EPS = 1e-5
DEFAULT_MAX_ITER = 100
MAX_D = 280
PROBLEM = np.dtype([('fold', '<i4'), ('cls', '<i4'), ('c', '<f4')])
RESULT = np.dtype([('iterations', '<i4'), ('converged', '<i4'), ('grad_ratio', '<f8')])
_WS = workspace.Scratch()      # the solver's scratch, one buffer per (device, stream)


def stratified_folds(labels, k=5):
    """Fold id of every sample as sklearn's `StratifiedKFold(k)` (no shuffling) assigns them, int32 [N], on the host.

    Classes are taken in order of first appearance; sample j of a class, in dataset order, gets the fold ids
    `arange(k).repeat(allocation[:, class])` with `allocation[f, c] = bincount(y_sorted[f::k])[c]`.  A class with fewer members
    than folds is refused."""
    y = np.asarray(labels)
    if y.ndim != 1 or y.shape[0] < 1:
        raise ValueError('labels must be a non-empty 1-D array')
    if isinstance(k, bool) or int(k) != k or k < 2:
        raise ValueError('k must be an integer >= 2 (got %r)' % (k,))
    k = int(k)
    _, first, inverse = np.unique(y, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(len(first))          # class -> its order of first appearance
    enc = rank[inverse]
    counts = np.bincount(enc)
    if counts.min() < k:
        raise ValueError('the least populated class has %d members: fewer than the %d folds' % (counts.min(), k))
    order = np.sort(enc)
    allocation = np.stack([np.bincount(order[f::k], minlength=len(first)) for f in range(k)])
    folds = np.empty(y.shape[0], np.int32)
    for c in range(len(first)):
        folds[enc == c] = np.arange(k, dtype=np.int32).repeat(allocation[:, c])
    return folds


def problem_table(folds, classes, Cs):
    """The solver's table, one row (fold, class, C) per problem.  fold -1 trains on every row."""
    folds, classes, Cs = np.asarray(folds), np.asarray(classes), np.asarray(Cs, np.float64)
    if not (folds.ndim == classes.ndim == Cs.ndim == 1 and len(folds) == len(classes) == len(Cs) and len(Cs) > 0):
        raise ValueError('folds, classes and Cs must be 1-D arrays of one length >= 1')
    if not (np.isfinite(Cs).all() and (Cs > 0).all()):
        raise ValueError('every C must be finite and > 0')
    t = np.empty(len(Cs), PROBLEM)
    t['fold'], t['cls'], t['c'] = folds, classes, Cs
    return t


def _check_x(x):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('x must be a 2-D tensor')
    if x.dtype != torch.float32:
        raise TypeError('x must be float32 (got %s)' % x.dtype)
    if not x.is_contiguous():
        raise ValueError('x must be contiguous')
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError('x is empty')
    if x.shape[1] > MAX_D:
        raise ValueError('x has %d features: at most %d are supported' % (x.shape[1], MAX_D))
    if not x.is_cuda:
        raise RuntimeError('finetune has no CPU path: x must live on a HIP device (got %s)' % x.device)


def _rows(name, t, n, device):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError('%s must be a 1-D array of %d integers' % (name, n))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError('%s must hold integers (got %s)' % (name, t.dtype))
    return t.to(device=device, dtype=torch.int32).contiguous()


def _table(problems):
    if isinstance(problems, np.ndarray) and problems.dtype == PROBLEM:
        t = np.ascontiguousarray(problems)
        if t.ndim != 1 or len(t) < 1:
            raise ValueError('the problem table is empty')
        if not (np.isfinite(t['c']).all() and (t['c'] > 0).all()):
            raise ValueError('every C must be finite and > 0')
        return t
    return problem_table(*problems)


def _check_solver_args(eps, max_iter):
    if not 0.0 < float(eps) < 1.0:
        raise ValueError('eps must lie in (0, 1) (got %r)' % (eps,))
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 0:
        raise ValueError('max_iter must be an integer >= 0 (got %r)' % (max_iter,))


def _fit(x, lab, fold, table, eps, max_iter):
    n, d = x.shape
    p = len(table)
    dev = x.device
    lib = _lib.load()
    prob = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    w = torch.empty(p, d + 1, dtype=torch.float32, device=dev)
    res = torch.empty(p * RESULT.itemsize, dtype=torch.uint8, device=dev)
    nbytes = lib.node_svm_workspace_bytes(n, d, p)
    if nbytes == 0:
        _lib.unsupported()
    with torch.cuda.device(dev):
        ptr = workspace.aligned_ptr(_WS.take(dev, nbytes))
        _lib.check(lib.node_svm_fit(n, d, p, x.data_ptr(), lab.data_ptr(), fold.data_ptr(), prob.data_ptr(), float(eps),
                                    int(max_iter), w.data_ptr(), res.data_ptr(), ptr, nbytes,
                                    torch.cuda.current_stream(dev).cuda_stream))
    return w, prob, res.cpu().numpy().view(RESULT)


def _score(x, lab, fold, prob, w, groups, neg_class, want_pred):
    n, d = x.shape
    g, k = groups.shape
    dev = x.device
    gd = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(dev)
    counts = torch.empty(2, g, dtype=torch.int32, device=dev)
    pred = torch.empty(g, n, dtype=torch.int32, device=dev) if want_pred else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.node_svm_cv_score(n, d, w.shape[0], g, k, x.data_ptr(), lab.data_ptr(), fold.data_ptr(), prob.data_ptr(),
                                         w.data_ptr(), gd.data_ptr(), int(neg_class), counts[0].data_ptr(), counts[1].data_ptr(),
                                         pred.data_ptr() if want_pred else None, torch.cuda.current_stream(dev).cuda_stream))
    counts = counts.cpu().numpy()
    return counts[0], counts[1], pred.cpu().numpy() if want_pred else None


def svc_cv_score(x, labels, row_fold, problems, weights, groups, neg_class=0, return_pred=False):
    """Held-out predictions of fitted problems.  `groups [G, K]` lists, per group, the K problems (indices into `problems`, one
    per class in class order, all of one fold) whose decision values compete: every row that the group's fold holds out is
    given the class of the first maximum (K = 1: the problem's class iff its decision value is > 0, else `neg_class`).
    Returns the integer counts `correct [G]` and `held [G]`, and with `return_pred` the predictions `[G, N]` (-1 where the
    row is not held out)."""
    _check_x(x)
    table = _table(problems)
    groups = np.asarray(groups)
    if groups.ndim != 2 or groups.size < 1 or groups.min() < 0 or groups.max() >= len(table):
        raise ValueError('groups must be a non-empty [G, K] array of indices into the %d problems' % len(table))
    if not (torch.is_tensor(weights) and weights.dtype == torch.float32 and weights.is_contiguous() and weights.device == x.device
            and tuple(weights.shape) == (len(table), x.shape[1] + 1)):
        raise ValueError('weights must be a contiguous float32 [%d, %d] tensor on %s' % (len(table), x.shape[1] + 1, x.device))
    lab = _rows('labels', labels, x.shape[0], x.device)
    fold = _rows('row_fold', row_fold, x.shape[0], x.device)
    prob = torch.from_numpy(table.view(np.uint8).copy()).to(x.device)
    correct, held, pred = _score(x, lab, fold, prob, weights, groups, neg_class, return_pred)
    return (correct, held, pred) if return_pred else (correct, held)


def linear_svc_fit(x, labels, row_fold, problems, eps=DEFAULT_EPS, max_iter=DEFAULT_MAX_ITER):
    """The raw solver: every problem of `problems` (a `problem_table`, or a (folds, classes, Cs) triple) over `x [N, D]`.
    Problem p trains on the rows with `row_fold != fold_p`, target +1 where `labels == cls_p`.  Returns the weights
    `[P, D + 1]` (float32, device; column D is the intercept) and a record array with `iterations`, `converged` and
    `grad_ratio` (|grad f(w)| / |grad f(0)| at the end) per problem."""
    _check_solver_args(eps, max_iter)
    _check_x(x)
    table = _table(problems)
    lab = _rows('labels', labels, x.shape[0], x.device)
    fold = _rows('row_fold', row_fold, x.shape[0], x.device)
    w, _, info = _fit(x, lab, fold, table, eps, max_iter)
    return w, info


def linear_svc_cv(x, labels, Cs=np.logspace(-2, 2, 5), folds=5, eps=DEFAULT_EPS, max_iter=DEFAULT_MAX_ITER):
    """`GridSearchCV(LinearSVC(), {'C': Cs}, cv=folds, scoring='accuracy')` with the refit, in one batch on the device.

    Returns an object with `mean_test_score [|Cs|]`, `fold_scores [folds, |Cs|]`, `fold_correct` and `fold_sizes` (the integer
    counts behind them), `best_index`, `best_C`, `best_score`, the refit at the best C as `coef [K', D]` and `intercept [K']`
    (K' = 1 for two classes, as in sklearn), `classes`, and per problem `n_iter`, `converged`, `grad_ratio`, with `problems`
    and `weights` (device) for every problem solved."""
    _check_solver_args(eps, max_iter)
    _check_x(x)
    Cs = np.asarray(Cs, np.float64)
    if Cs.ndim != 1 or len(Cs) < 1 or not (np.isfinite(Cs).all() and (Cs > 0).all()):
        raise ValueError('Cs must be a non-empty 1-D array of finite values > 0')
    n, d = x.shape
    lab = _rows('labels', labels, n, x.device)
    y = lab.cpu().numpy()
    classes = np.unique(y)
    if len(classes) < 2:
        raise ValueError('the labels hold %d class: at least 2 are needed' % len(classes))
    row_fold = stratified_folds(y, folds)
    targets = classes[1:] if len(classes) == 2 else classes
    k = len(targets)
    fold_list = list(range(int(folds))) + [-1]
    table = problem_table(np.repeat(fold_list, len(Cs) * k), np.tile(targets, len(fold_list) * len(Cs)),
                          np.tile(np.repeat(Cs, k), len(fold_list)))
    fold_d = torch.from_numpy(row_fold).to(x.device)
    w, prob, info = _fit(x, lab, fold_d, table, eps, max_iter)
    n_groups = int(folds) * len(Cs)
    groups = np.arange(n_groups * k).reshape(n_groups, k)                         # the table is ordered (fold, C, class)
    correct, held, _ = _score(x, lab, fold_d, prob, w, groups, int(classes[0]), False)
    counts = np.stack([correct, held]).reshape(2, int(folds), len(Cs))
    fold_scores = counts[0] / counts[1]
    mean = fold_scores.mean(0)
    best = int(np.argmax(mean))                                   # the first maximum: the smallest C among equals
    refit = n_groups * k + best * k
    wb = w[refit:refit + k].cpu().numpy()
    converged = info['converged'].astype(bool)
    if not converged.all():
        warnings.warn('%d of %d SVM problems did not converge within %d Newton iterations (largest gradient ratio %.2e)'
                      % ((~converged).sum(), len(table), max_iter, info['grad_ratio'][~converged].max()), RuntimeWarning)
    return types.SimpleNamespace(mean_test_score=mean, fold_scores=fold_scores, fold_correct=counts[0], fold_sizes=counts[1],
                                 best_index=best, best_C=float(Cs[best]), best_score=float(mean[best]), coef=wb[:, :d].copy(),
                                 intercept=wb[:, d].copy(), classes=classes, n_iter=info['iterations'].copy(), converged=converged,
                                 grad_ratio=info['grad_ratio'].copy(), problems=table, weights=w, Cs=Cs, row_fold=row_fold)


def predict(coef, intercept, classes, x):
    """Class predictions of a fitted search on host features `x [N, D]` (numpy), as `LinearSVC.predict` forms them."""
    z = np.asarray(x, np.float64) @ np.asarray(coef, np.float64).T + np.asarray(intercept, np.float64)
    classes = np.asarray(classes)
    if z.shape[1] == 1:
        return classes[(z[:, 0] > 0).astype(np.int64)]
    return classes[z.argmax(1)]

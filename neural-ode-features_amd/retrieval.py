"""Retrieval evaluation on the HIP backend: per-query average precision (AP) and AP@k of a database ranked by inner
product, the metrics of `evaluate.py retrieval` in the reference (evaluate.py:308-361), which calls sklearn's
`average_precision_score` once per query on the host.

    ap, ap_k = average_precision(queries, db, query_labels, db_labels, k=10)

Scores come from the fp32 matrix pipe, each query's ranking is sorted in LDS by one workgroup (csrc/kernels_retrieval.hip).
AP follows sklearn exactly: equal scores form one threshold, a query with no relevant item gets 0.0.  AP@k takes the top k
by score, and among equal scores the higher database index ranks first (a stable argsort reversed: numpy leaves the
order of `argsort()[::-1]` unspecified there).  Results are float64 device tensors enqueued on the current stream, with
no host synchronisation; they are bit-identical from run to run.  The database holds at most MAX_DB items.
"""
from __future__ import annotations

import torch

from . import _lib, workspace

MAX_DB = 16384
_WS = workspace.Scratch()      # the score chunk, one buffer per (device, stream)


def _check_matrix(name, t):
    if not torch.is_tensor(t) or t.dim() != 2:
        raise ValueError('%s must be a 2-D tensor' % name)
    if t.dtype != torch.float32:
        raise TypeError('%s must be float32 (got %s)' % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)


def _check_device(name, t):
    if not t.is_cuda:
        raise RuntimeError('retrieval has no CPU path: %s must live on a HIP device (got %s)' % (name, t.device))


def _labels(name, t, n, device):
    if not torch.is_tensor(t) or t.dim() != 1 or t.shape[0] != n:
        raise ValueError('%s must be a 1-D tensor of %d labels' % (name, n))
    if t.device != device:
        raise RuntimeError('%s must live on %s (got %s)' % (name, device, t.device))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError('%s must hold integer labels (got %s)' % (name, t.dtype))
    return t.to(torch.int32).contiguous()


def _check_k(k):
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError('k must be an integer >= 1 (got %r)' % (k,))


def _check_db(nd):
    if nd > MAX_DB:
        raise ValueError('the database holds %d items: at most %d are supported' % (nd, MAX_DB))
    if nd < 1:
        raise ValueError('the database is empty')


def average_precision_from_scores(scores, query_labels, db_labels, k=10):
    """AP and AP@k of every row of a given score matrix `scores [Nq, Nd]` (the ranking stage alone)."""
    _check_k(k)
    _check_matrix('scores', scores)
    nq, nd = scores.shape
    _check_db(nd)
    _check_device('scores', scores)
    ql = _labels('query_labels', query_labels, nq, scores.device)
    xl = _labels('db_labels', db_labels, nd, scores.device)
    ap = torch.empty(nq, dtype=torch.float64, device=scores.device)
    ap_k = torch.empty_like(ap)
    if nq == 0:
        return ap, ap_k
    lib = _lib.load()
    with torch.cuda.device(scores.device):
        _lib.check(lib.node_rank_ap(nq, nd, scores.data_ptr(), ql.data_ptr(), xl.data_ptr(), int(k), ap.data_ptr(),
                                    ap_k.data_ptr(), None, 0, torch.cuda.current_stream(scores.device).cuda_stream))
    return ap, ap_k


def average_precision(queries, db, query_labels, db_labels, k=10):
    """Per-query AP and AP@k of `db [Nd, D]` ranked by the inner product with each row of `queries [Nq, D]`; an item is
    relevant when its label equals the query's.  Returns two float64 device tensors [Nq]."""
    _check_k(k)
    _check_matrix('queries', queries)
    _check_matrix('db', db)
    nq, d = queries.shape
    nd = db.shape[0]
    if db.shape[1] != d:
        raise ValueError('queries have %d features, the database %d' % (d, db.shape[1]))
    if d < 1:
        raise ValueError('the features are empty')
    _check_db(nd)
    _check_device('queries', queries)
    if db.device != queries.device:
        raise RuntimeError('queries and db must live on the same device (%s, %s)' % (queries.device, db.device))
    ql = _labels('query_labels', query_labels, nq, queries.device)
    xl = _labels('db_labels', db_labels, nd, queries.device)
    ap = torch.empty(nq, dtype=torch.float64, device=queries.device)
    ap_k = torch.empty_like(ap)
    if nq == 0:
        return ap, ap_k
    lib = _lib.load()
    nbytes = lib.node_retrieval_workspace_bytes(nq, nd, d)
    with torch.cuda.device(queries.device):
        ptr = workspace.aligned_ptr(_WS.take(queries.device, nbytes))
        _lib.check(lib.node_retrieval_ap(nq, nd, d, queries.data_ptr(), db.data_ptr(), ql.data_ptr(), xl.data_ptr(), int(k),
                                         ap.data_ptr(), ap_k.data_ptr(), ptr, nbytes,
                                         torch.cuda.current_stream(queries.device).cuda_stream))
    return ap, ap_k

"""GPU: the retrieval evaluation (csrc/kernels_retrieval.hip, retrieval.py, `evaluate.py retrieval`) against the function the
reference calls, sklearn.metrics.average_precision_score (evaluate.py:308-361)."""
import warnings

import numpy as np
import pytest
import sklearn.metrics as sklearn_metrics
import torch

pytestmark = pytest.mark.gpu


def _sk_ap(gt, s):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # "No positive class found in y_true": sklearn returns 0.0 there
        return float(sklearn_metrics.average_precision_score(gt, s))


def _sk_ap_k(gt, s, k):
    """evaluate.py:343-346 with the tie order pinned: the stable ascending argsort, reversed."""
    r = s.argsort(kind='stable')[::-1][:k]
    return _sk_ap(gt[r], s[r])


def _rows(nd, rng):
    """Score rows that stress the ranking: continuous, quantised (heavy ties, also at the k boundary), -0.0 beside +0.0,
    all equal."""
    rows = [rng.standard_normal(nd).astype(np.float32),
            rng.integers(-2, 3, nd).astype(np.float32),
            (rng.integers(0, 3, nd) * 0.5).astype(np.float32),
            np.where(rng.random(nd) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32),
            np.full(nd, 0.25, np.float32)]
    mixed = np.where(rng.random(nd) < 0.3, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    mixed[rng.random(nd) < 0.3] = 1.0
    mixed[rng.random(nd) < 0.2] = -1.0
    rows.append(mixed)
    return np.stack(rows)


@pytest.mark.parametrize('nd', [1, 2, 7, 1000, 10000, 16384])
def test_ranking_stage_matches_sklearn(nd):
    from neural_ode_features_amd.retrieval import average_precision_from_scores
    rng = np.random.default_rng(nd)
    dev = torch.device('cuda')
    s = _rows(nd, rng)
    nrow = s.shape[0]
    xl = rng.integers(0, 3, nd).astype(np.int32)
    ql = rng.integers(0, 3, nrow).astype(np.int32)
    ql[-1] = 7                                   # a query with no relevant item: 0.0
    # second call: every item relevant (1.0), and one query with none
    xl_all = np.zeros(nd, np.int32)
    ql_all = np.zeros(nrow, np.int32)
    ql_all[0] = 1
    sd = torch.from_numpy(s).to(dev)
    for qlab, xlab in ((ql, xl), (ql_all, xl_all)):
        gt = qlab[:, None] == xlab[None, :]
        want = [_sk_ap(gt[i], s[i]) for i in range(nrow)]
        for k in sorted({1, 10, nd, nd + 5}):
            ap, ap_k = average_precision_from_scores(sd, torch.from_numpy(qlab).to(dev), torch.from_numpy(xlab).to(dev), k=k)
            ap, ap_k = ap.cpu().numpy(), ap_k.cpu().numpy()
            for i in range(nrow):
                assert abs(ap[i] - want[i]) <= 1e-12, (nd, k, i, ap[i], want[i])
                wk = _sk_ap_k(gt[i], s[i], k)
                assert abs(ap_k[i] - wk) <= 1e-12, (nd, k, i, ap_k[i], wk)
    # the closed forms the reference's semantics give
    gt = ql[:, None] == xl[None, :]
    ap, _ = average_precision_from_scores(sd, torch.from_numpy(ql).to(dev), torch.from_numpy(xl).to(dev))
    ap = ap.cpu().numpy()
    assert ap[-1] == 0.0
    assert abs(ap[4] - gt[4].sum() / nd) <= 1e-12               # all-equal scores: one threshold, AP = P / Nd
    ap, _ = average_precision_from_scores(sd, torch.from_numpy(ql_all).to(dev), torch.from_numpy(xl_all).to(dev))
    ap = ap.cpu().numpy()
    assert ap[0] == 0.0 and (ap[1:] == 1.0).all()


def test_fused_path_exact_on_integer_features():
    """Integer features in [-4, 4] at D = 256: every dot product is an integer below 2^24, exact in fp32 whatever the
    summation order, so the fused scores are the float64 scores and AP / AP@10 must match sklearn to 1e-12, ties and all."""
    from neural_ode_features_amd.retrieval import average_precision
    rng = np.random.default_rng(11)
    nq, nd, d = 3000, 10000, 256
    q = rng.integers(-4, 5, (nq, d)).astype(np.float32)
    x = rng.integers(-4, 5, (nd, d)).astype(np.float32)
    ql = rng.integers(0, 10, nq).astype(np.int32)
    xl = rng.integers(0, 10, nd).astype(np.int32)
    dev = torch.device('cuda')
    ap, ap_k = average_precision(torch.from_numpy(q).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(ql).to(dev),
                                 torch.from_numpy(xl).to(dev), k=10)
    ap, ap_k = ap.cpu().numpy(), ap_k.cpu().numpy()
    s = q.astype(np.float64) @ x.astype(np.float64).T
    ties = 0
    for i in range(nq):
        gt = xl == ql[i]
        assert abs(ap[i] - _sk_ap(gt, s[i])) <= 1e-12, i
        assert abs(ap_k[i] - _sk_ap_k(gt, s[i], 10)) <= 1e-12, i
        ties += len(np.unique(s[i])) < nd
    assert ties == nq                            # the data exercises tie groups in every row


def _reference_normalised(n, d, rng):
    f = rng.standard_normal((n, d)).astype(np.float32)
    return f / (np.linalg.norm(f, axis=-2, keepdims=True) + 1e-7)          # evaluate.py:326, as the reference writes it


def test_fused_path_on_continuous_features():
    """Gaussian features normalised as the reference does, against sklearn on numpy's float32 `queries.dot(db.T)`.  Both
    scores are fp32 sums of the same exact products in different orders, so only near-ties can rank differently.  A swap
    of two adjacent items at rank r moves AP by at most 1 / (P r) (P ~ 200 relevant items here): per query 2e-3 allows a
    few swaps near the top, the mean 1e-5 allows them only rarely.  AP@10 changes only when a near-tie straddles the
    boundary: at most 1 % of the queries differ by more than the 1e-12 of a different fp64 summation, mean 1e-3."""
    from neural_ode_features_amd.retrieval import average_precision
    rng = np.random.default_rng(5)
    n, d = 2000, 64
    f = _reference_normalised(n, d, rng)
    y = rng.integers(0, 10, n).astype(np.int32)
    dev = torch.device('cuda')
    fd, yd = torch.from_numpy(f).to(dev), torch.from_numpy(y).to(dev)
    ap, ap_k = average_precision(fd, fd, yd, yd, k=10)
    ap, ap_k = ap.cpu().numpy(), ap_k.cpu().numpy()
    s = f.dot(f.T)
    gt = y[:, None] == y[None, :]
    want = np.array([_sk_ap(gt[i], s[i]) for i in range(n)])
    want_k = np.array([_sk_ap_k(gt[i], s[i], 10) for i in range(n)])
    err, err_k = np.abs(ap - want), np.abs(ap_k - want_k)
    assert err.max() <= 2e-3 and err.mean() <= 1e-5, (err.max(), err.mean())
    assert (err_k > 1e-12).mean() <= 0.01 and err_k.mean() <= 1e-3, ((err_k > 1e-12).mean(), err_k.mean())


def test_outputs_are_bit_identical_from_run_to_run():
    from neural_ode_features_amd.retrieval import average_precision
    rng = np.random.default_rng(9)
    n, d = 10000, 256
    dev = torch.device('cuda')
    f = torch.from_numpy(_reference_normalised(n, d, rng)).to(dev)
    y = torch.from_numpy(rng.integers(0, 10, n).astype(np.int32)).to(dev)
    a1, k1 = average_precision(f, f, y, y, k=10)
    a2, k2 = average_precision(f, f, y, y, k=10)
    assert torch.equal(a1, a2) and torch.equal(k1, k2)
    assert float(a1.min()) > 0.0 and float(a1.max()) <= 1.0


def test_retrieval_mode_end_to_end(tmp_path):
    """train -> features -> retrieval on a run directory, every column against a numpy + sklearn restatement of
    evaluate.py:318-361 applied to each tolerance slice of the same features.npz (bounds of the continuous-feature test)."""
    import pandas as pd
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    run = str(tmp_path / 'run')
    assert T.main(['--dataset', 'mnist', '-f', '16', '-b', '32', '--synthetic-size', '1200', '-a', '--lr', '0.05', '-e', '1',
                   '--run-dir', run]) == 0
    E.main(['features', run, '--t1', '0', '0.5', '1', '--tol', '1e-3', '1e-1', '--limit', '300'])
    out = E.main(['retrieval', run])
    df = pd.read_csv(out)
    assert list(df.columns) == ['ap_asym', 'ap_sym', 'ap10_asym', 'ap10_sym', 't1', 'tol']
    assert len(df) == 2 * 3 * 300
    z = np.load(tmp_path / 'run' / 'features.npz')
    feats, y_true, t1s, tols = z['features'], z['y_true'], z['t1s'], z['tols']
    assert feats.shape == (2, 3, 300, 16)
    feats = feats / (np.linalg.norm(feats, axis=-2, keepdims=True) + 1e-7)
    n = feats.shape[-2]
    gt = np.broadcast_to(y_true, (n, n)) == y_true[:n].reshape(n, -1)
    want = {c: [] for c in ('ap_asym', 'ap_sym', 'ap10_asym', 'ap10_sym', 't1', 'tol')}
    for ti, tol in enumerate(tols):
        f = feats[ti]
        for i, t1 in enumerate(t1s):
            for name, db in (('asym', f[-1]), ('sym', f[i])):
                s = f[i].dot(db.T)
                want['ap_' + name] += [_sk_ap(gt[j], s[j]) for j in range(n)]
                want['ap10_' + name] += [_sk_ap_k(gt[j], s[j], 10) for j in range(n)]
            want['t1'] += [t1] * n
            want['tol'] += [tol] * n
    assert np.array_equal(df.t1.to_numpy(), np.array(want['t1'])) and np.array_equal(df.tol.to_numpy(), np.array(want['tol']))
    for c in ('ap_asym', 'ap_sym'):
        err = np.abs(df[c].to_numpy() - np.array(want[c]))
        assert err.max() <= 2e-3 and err.mean() <= 1e-5, (c, err.max(), err.mean())
    for c in ('ap10_asym', 'ap10_sym'):
        err = np.abs(df[c].to_numpy() - np.array(want[c]))
        assert (err > 1e-12).mean() <= 0.01 and err.mean() <= 1e-3, (c, (err > 1e-12).mean(), err.mean())

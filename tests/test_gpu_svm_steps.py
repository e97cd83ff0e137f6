"""GPU: the finetune solver's kernels (csrc/kernels_svm.hip, launch sequence csrc/svm_api.hip) step by step against the fp64
restatement of tests/svm_reference.py, and the scoring kernel against exact integer arithmetic.

tests/test_gpu_finetune.py holds the solver to its end result.  A truncated Newton method corrects its own errors, so that check
sees the gradient product and little else: a wrong Hessian-vector product, X~ s product, CG update or line search only costs
iterations.  Here the trajectory is opened from outside.  Runs are bit-identical, so `linear_svc_fit(..., max_iter=k)` for
k = 0, 1, 2, ... returns the iterates w_k of ONE trajectory with grad_ratio = |g(w_k)| / |g(0)|, and each step is compared with
`newton_step` from the DEVICE's own previous iterate:

  * prefix consistency of the runs; the reported gradient ratio against the fp64 gradient at every device iterate;
  * w_1 element by element (all Cs), w_2 at C <= 1 (the Hessian-vector product on a real active set);
  * descent of the fp64 objective; Newton iteration counts against both restatements; every problem converges;
  * degenerate problems; the chunked path of node_svm_fit against unchunked fits, bit for bit;
  * k_svm_cv_score on given integer weights (exact), with exact ties, z == 0 at K = 1, empty groups and pred == NULL.

The shapes (svm_reference.CASES) sit on the edges of the tiling: 64 problems per tile, 64-row slabs, 32-column tiles of D + 1 padded
to even, MAXQ = 5 column tiles per wave (D = 280: 18 tiles), 256-row line-search groups.

Tolerances: 8 x the deviation of the fp32-storage restatement from the fp64 one from the same iterate (svm_reference.SVM_DEV_*,
measured and kept true by tests/test_svm_reference_host.py) -- the kernels sum in another order.  A problem is left out of a step
comparison only where a decision of the restatement is thin (svm_reference.thin); at most 20 % per case, asserted.  Measured on an
MI355X: profiles/finetune_steps.txt.
"""
import functools

import numpy as np
import pytest
import torch

from tests import svm_reference as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(c) for c in R.CASES]
MAX_PREFIX = 8
TOL_STEP1 = 8 * R.SVM_DEV_STEP1          # 5.6e-5 of max|w_1|
TOL_STEP2 = 8 * R.SVM_DEV_STEP2          # 8.8e-3 of max|w_2 - w_1|
TOL_RATIO = 8 * R.SVM_DEV_RATIO          # 8e-7 absolute


def _fit(x, labels, row_fold, table, **kw):
    from neural_ode_features_amd.finetune import linear_svc_fit
    dev = torch.device('cuda')
    w, info = linear_svc_fit(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(row_fold).to(dev), table, **kw)
    return w.cpu().numpy(), info


def _table(folds, classes, cs):
    from neural_ode_features_amd.finetune import problem_table
    return problem_table(folds, classes, cs)


@functools.lru_cache(maxsize=None)
def _runs(case):
    """The full fit and the prefixes max_iter = 0 .. min(final iterations, 8) of a case, once, shared by the tests (read only)."""
    cd = R.case_data(case)
    table = _table(cd.folds, cd.classes, cd.cs)
    full = _fit(cd.x, cd.labels, cd.row_fold, table)
    k_max = min(int(full[1]['iterations'].max()), MAX_PREFIX)
    return full, [_fit(cd.x, cd.labels, cd.row_fold, table, max_iter=k) for k in range(k_max + 1)]


def _g0(prob):
    xt, y, c = prob
    return float(np.linalg.norm(R.gradient(np.zeros(xt.shape[1]), xt, y, c)))


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_prefixes_of_one_trajectory(case):
    (w_full, info_full), runs = _runs(case)
    final = info_full['iterations']
    for k, (w, info) in enumerate(runs):
        assert np.array_equal(info['iterations'], np.minimum(k, final)), k
        stopped = final <= k
        assert np.array_equal(w[stopped].view(np.int32), w_full[stopped].view(np.int32)), k
        assert np.array_equal(info[stopped], info_full[stopped]), k
        assert not info['converged'][~stopped].any(), k
    assert not runs[0][0].any()


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_reported_gradient_ratio_is_the_fp64_gradient_at_the_device_iterate(case):
    cd = R.case_data(case)
    _, runs = _runs(case)
    worst = 0.0
    for k, (w, info) in enumerate(runs):
        for p, (xt, y, c) in enumerate(cd.problems):
            want = float(np.linalg.norm(R.gradient(w[p].astype(np.float64), xt, y, c))) / _g0(cd.problems[p])
            err = abs(info['grad_ratio'][p] - want)
            worst = max(worst, err)
            assert err <= TOL_RATIO, (k, p, c, info['grad_ratio'][p], want)
    print('STEPS %s grad_ratio: error %.3g (bound %.3g) over %d runs' % (R.case_id(case), worst, TOL_RATIO, len(runs)))


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_first_newton_step_element_by_element(case):
    cd = R.case_data(case)
    _, runs = _runs(case)
    w1 = runs[1][0].astype(np.float64)
    worst, left_out = 0.0, 0
    for p, (xt, y, c) in enumerate(cd.problems):
        st = R.newton_step(np.zeros(xt.shape[1]), xt, y, c, None)
        if st.cg_margin < R.MARGIN:
            left_out += 1
            continue
        err = np.abs(w1[p] - st.w_next).max() / np.abs(st.w_next).max()
        worst = max(worst, err)
        assert err <= TOL_STEP1, (p, c, err, st.cg_iters, st.t)
    print('STEPS %s step 1: error %.3g (bound %.3g), left out %d of %d' % (R.case_id(case), worst, TOL_STEP1, left_out, cd.p))
    assert left_out <= R.EXCLUDED_CAP * cd.p


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_second_newton_step_from_the_device_iterate(case):
    cd = R.case_data(case)
    (_, info_full), runs = _runs(case)
    assert len(runs) > 2
    w1, w2 = runs[1][0].astype(np.float64), runs[2][0].astype(np.float64)
    worst, left_out, compared = 0.0, 0, 0
    for p, (xt, y, c) in enumerate(cd.problems):
        if c > 1.0 or info_full['iterations'][p] < 2:
            continue
        compared += 1
        st = R.newton_step(w1[p], xt, y, c, _g0(cd.problems[p]))
        if R.thin(st):
            left_out += 1
            continue
        err = np.abs(w2[p] - st.w_next).max() / np.abs(st.w_next - w1[p]).max()
        worst = max(worst, err)
        assert err <= TOL_STEP2, (p, c, err, st.cg_iters, st.t)
    print('STEPS %s step 2: error %.3g (bound %.3g), left out %d of %d' % (R.case_id(case), worst, TOL_STEP2, left_out, compared))
    assert 2 * compared >= (cd.cs <= 1.0).sum(), compared
    assert left_out <= R.EXCLUDED_CAP * compared


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_every_step_descends(case):
    cd = R.case_data(case)
    (_, info_full), runs = _runs(case)
    steps = 0
    for k in range(len(runs) - 1):
        (w0, info0), (w1, _) = runs[k], runs[k + 1]
        for p, (xt, y, c) in enumerate(cd.problems):
            if info_full['iterations'][p] > k and info0['grad_ratio'][p] >= 1e-3:
                f0, f1 = R.objective(w0[p].astype(np.float64), xt, y, c), R.objective(w1[p].astype(np.float64), xt, y, c)
                steps += 1
                assert f1 < f0, (k, p, c, f0, f1)
    assert steps >= cd.p


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_newton_iteration_counts(case):
    cd = R.case_data(case)
    (_, info), _ = _runs(case)
    assert info['converged'].all(), (info['iterations'].max(), info['grad_ratio'].max())
    s64, s32 = R.case_solutions(case, 'f64'), R.case_solutions(case, 'f32')
    got = info['iterations']
    it64, it32 = np.array([s.iterations for s in s64]), np.array([s.iterations for s in s32])
    low = cd.cs <= 1.0
    print('STEPS %s iterations: device <= %d, fp64 <= %d, fp32 <= %d; C <= 1: device - fp64 in [%d, %d]; C = 100: device - fp32 in [%s]'
          % (R.case_id(case), got.max(), it64.max(), it32.max(), (got - it64)[low].min(), (got - it64)[low].max(),
             ', '.join('%d' % v for v in ((got - it32)[~low].min(), (got - it32)[~low].max())) if (~low).any() else ''))
    assert (np.abs(got - it64)[low] <= 1).all(), (got[low], it64[low])
    assert (got[~low] <= it32[~low] + R.SVM_ITER_GAP_C100 + 2).all(), (got[~low], it32[~low])


def test_degenerate_problems():
    """On the (37, 1) data: a class no row has, a fold no row carries, and (with every row in fold 0) a fold that holds out all."""
    cd = R.case_data(R.CASES[0])
    folds = np.array([-1, 7, 0, 7, -1, 3], np.int32)
    classes = np.array([0, 0, 9, 9, 9, 9], np.int32)
    cs = np.array([1.0, 1.0, 1.0, 100.0, 100.0, 0.01])
    table = _table(folds, classes, cs)
    w, info = _fit(cd.x, cd.labels, cd.row_fold, table)
    w1, _ = _fit(cd.x, cd.labels, cd.row_fold, table, max_iter=1)
    assert info['converged'].all()
    # a fold that no row carries trains on every row: the fold -1 problem, bit for bit
    assert np.array_equal(w[1].view(np.int32), w[0].view(np.int32)) and info[1] == info[0]
    assert np.array_equal(w[3].view(np.int32), w[4].view(np.int32)) and info[3] == info[4]
    # an absent class: every target is -1, the threshold is eps max(min(0, n), 1) / n |g(0)|; the first step and the end against the
    # restatement.  f is 1-strongly convex, so |w - w*| <= |g(w)|: both ends lie within their own fp64 gradient norm of w*
    for p in range(2, 6):
        xt, y, c = R.problem(cd.x, cd.labels, cd.row_fold, folds[p], classes[p], cs[p])
        assert (y == -1.0).all()
        g0 = _g0((xt, y, c))
        st = R.newton_step(np.zeros(2), xt, y, c, None)
        assert st.cg_margin >= R.MARGIN
        assert np.abs(w1[p] - st.w_next).max() <= TOL_STEP1 * np.abs(st.w_next).max(), p
        sol = R.solve(xt, y, c)
        assert sol.converged
        if c <= 1.0:
            assert abs(int(info['iterations'][p]) - sol.iterations) <= 1
        else:
            assert info['iterations'][p] <= R.solve(xt, y, c, storage=np.float32).iterations + R.SVM_ITER_GAP_C100 + 2
        g_dev = float(np.linalg.norm(R.gradient(w[p].astype(np.float64), xt, y, c)))
        assert abs(info['grad_ratio'][p] - g_dev / g0) <= TOL_RATIO
        assert g_dev / g0 <= R.DEFAULT_EPS / len(y) + TOL_RATIO
        g_ref = float(np.linalg.norm(R.gradient(sol.w, xt, y, c)))
        assert np.linalg.norm(w[p] - sol.w) <= g_dev + g_ref
        assert w[p][1] < 0.0 and w[p][0] <= 0.0          # features are >= 0, targets -1: nothing pulls a weight up
    # every row held out: nothing to train on
    table = _table([0, -1], [0, 0], [1.0, 1.0])
    w, info = _fit(cd.x, cd.labels, np.zeros(cd.n, np.int32), table)
    assert not w[0].any() and info['converged'][0] == 1 and info['iterations'][0] == 0 and info['grad_ratio'][0] == 0.0
    assert w[1].any() and info['converged'][1] == 1 and info['iterations'][1] > 0


def test_chunked_fit_equals_unchunked_fits_bit_for_bit():
    """Z and X~ s of 4160 problems over 8192 rows exceed the workspace cap, so node_svm_fit runs them in chunks of whole tiles,
    offsetting `problems`, `weights` and `results`.

    The number of row groups of a launch, and with it the order of the fp32 sums, follows the number of problems in the launch
    (svm_plan): a problem's result does not depend on its column, but its last bits depend on how many problems run beside it.  So
    the chunked fit is bit-equal to unchunked fits of ITS OWN chunks, table[:pc] and table[pc:], where pc is read off the
    workspace size; the halves table[:2080] and table[2080:] run under another plan and are held to what 1-strong convexity
    gives two approximate minimisers of one problem, |w - w'| <= |g(w)| + |g(w')|, in fp64.  The reported gradient ratio
    against the fp64 gradient at the device's w ties every row of `weights` and `results` to its own row of the table."""
    from neural_ode_features_amd import _lib
    n, d, p = 8192, 1, 4160
    cap = 256 << 20
    assert 8 * n * p > cap and 8 * n * (p // 2) < cap
    size = _lib.load().node_svm_workspace_bytes
    assert size(n, d, p) <= cap and size(n, d, p // 2) < size(n, d, p) < 2 * size(n, d, p // 2)
    pc = min(q for q in range(64, p, 64) if size(n, d, q) == size(n, d, p))          # the chunk: the first size the workspace stops at
    assert p // 2 < pc < p and size(n, d, pc - 64) < size(n, d, pc)
    x, labels = R.make_data(n, d, 4, R.SEP, 5)
    row_fold = (np.arange(n) % 5).astype(np.int32)
    rows = [(f, k, c) for f in R.FOLDS for k in range(4) for c in np.geomspace(0.01, 10.0, 174)][:p]
    table = _table([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    w, info = _fit(x, labels, row_fold, table)
    assert info['converged'].all() and info['iterations'].min() >= 1
    for lo, hi in ((0, pc), (pc, p)):
        w_part, info_part = _fit(x, labels, row_fold, table[lo:hi])
        assert np.array_equal(w[lo:hi].view(np.int32), w_part.view(np.int32)), lo
        assert np.array_equal(info[lo:hi], info_part), lo
    w_half = np.concatenate([_fit(x, labels, row_fold, table[lo:hi])[0] for lo, hi in ((0, p // 2), (p // 2, p))])
    data = {}
    for q, (f, k, c) in enumerate(rows):
        if (f, k) not in data:
            data[f, k] = R.problem(x, labels, row_fold, f, k, 1.0)[:2]
        xt, y = data[f, k]
        c = float(table['c'][q])
        g0 = float(np.linalg.norm(R.gradient(np.zeros(2), xt, y, c)))
        g_dev = float(np.linalg.norm(R.gradient(w[q].astype(np.float64), xt, y, c)))
        assert abs(info['grad_ratio'][q] - g_dev / g0) <= TOL_RATIO, (q, info['grad_ratio'][q], g_dev / g0)
        g_half = float(np.linalg.norm(R.gradient(w_half[q].astype(np.float64), xt, y, c)))
        assert np.linalg.norm(w[q].astype(np.float64) - w_half[q]) <= g_dev + g_half, q


# ----------------------------------------------------------------------------------------------------------------------
# k_svm_cv_score on given weights.  Features and weights are small integers held in fp32: every fmaf of the kernel's chain is
# exact, so the expected class is exact integer arithmetic and ties are exact ties.
# ----------------------------------------------------------------------------------------------------------------------
SCORE_FOLDS = (0, 1, 2, 5)          # rows carry folds 0..2: the group of fold 5 holds nothing out
NEG_CLASS = 77


def _score_problem(n, d, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, (n, d)).astype(np.float32)
    classes = 3 + 2 * np.arange(k)
    labels = rng.choice(np.concatenate([classes, [NEG_CLASS, 1]]), n).astype(np.int32)
    row_fold = (np.arange(n) % 3).astype(np.int32)
    g = len(SCORE_FOLDS)
    order = rng.permutation(g * k)                                  # the groups' problems lie scattered over the table
    groups = order.reshape(g, k)
    w = rng.integers(-3, 4, (g * k, d + 1)).astype(np.float32)
    w[:, d] = rng.integers(-6, 7, g * k)
    if k >= 2:
        w[groups[0, k - 1]] = w[groups[0, 0]]                       # group 0: the first and the last class tie on every row
        w[groups[1]] = w[groups[1, 0]]                              # group 1: all classes tie on every row
    else:
        w[groups[1, 0]] = 0.0                                       # K = 1: z == 0 on every row
    pf, pc = np.zeros(g * k, np.int32), np.zeros(g * k, np.int32)
    for gi, fold in enumerate(SCORE_FOLDS):
        pf[groups[gi]], pc[groups[gi]] = fold, classes
    return x, labels, row_fold, groups, w, pf, pc


def _score_expected(x, labels, row_fold, groups, w, pf, pc):
    z = np.concatenate([x.astype(np.int64), np.ones((len(x), 1), np.int64)], 1) @ w.astype(np.int64).T          # [N, P], exact
    pred = np.full((len(groups), len(x)), -1, np.int64)
    for gi, gp in enumerate(groups):
        held = row_fold == pf[gp[0]]
        if len(gp) == 1:
            guess = np.where(z[:, gp[0]] > 0, pc[gp[0]], NEG_CLASS)
        else:
            guess = pc[gp][z[:, gp].argmax(1)]                      # numpy's argmax: the first maximum
        pred[gi, held] = guess[held]
    return (pred == labels[None]).sum(1), (pred >= 0).sum(1), pred


@pytest.mark.parametrize('k', [1, 2, 10])
@pytest.mark.parametrize('d', [1, 33, 280])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 700])
def test_cv_score_on_integer_weights_is_exact(n, d, k):
    from neural_ode_features_amd.finetune import svc_cv_score
    x, labels, row_fold, groups, w, pf, pc = _score_problem(n, d, k, 1000 * n + 10 * d + k)
    correct, held, pred = _score_expected(x, labels, row_fold, groups, w, pf, pc)
    assert held[3] == 0 and correct[3] == 0 and (pred[3] == -1).all()
    dev = torch.device('cuda')
    args = (torch.from_numpy(x).to(dev), labels, row_fold, _table(pf, pc, np.ones(len(pf))), torch.from_numpy(w).to(dev), groups)
    got = svc_cv_score(*args, neg_class=NEG_CLASS, return_pred=True)
    assert np.array_equal(got[2], pred)
    assert np.array_equal(got[0], correct) and np.array_equal(got[1], held)
    counts = svc_cv_score(*args, neg_class=NEG_CLASS)                 # pred == NULL
    assert len(counts) == 2 and np.array_equal(counts[0], correct) and np.array_equal(counts[1], held)


def test_cv_score_on_continuous_weights_against_fp64_argmax():
    from neural_ode_features_amd.finetune import svc_cv_score
    n, d, k = 700, 33, 10
    rng = np.random.default_rng(7)
    x, labels = R.make_data(n, d, k, R.SEP, 7)
    row_fold = (np.arange(n) % 5).astype(np.int32)
    w = rng.standard_normal((5 * k, d + 1)).astype(np.float32)
    pf, pc = np.repeat(np.arange(5), k).astype(np.int32), np.tile(np.arange(k), 5).astype(np.int32)
    groups = np.arange(5 * k).reshape(5, k)
    dev = torch.device('cuda')
    correct, held, pred = svc_cv_score(torch.from_numpy(x).to(dev), labels.astype(np.int32), row_fold, _table(pf, pc, np.ones(5 * k)),
                                       torch.from_numpy(w).to(dev), groups, return_pred=True)
    xt = np.concatenate([x.astype(np.float64), np.ones((n, 1))], 1)
    for f in range(5):
        rows = row_fold == f
        wf = w[groups[f]].astype(np.float64)
        z = xt[rows] @ wf.T
        bound = 2.0 * (d + 1) * 2.0 ** -24 * (np.abs(xt[rows]) @ np.abs(wf).T).max(1)          # |x|.|w| + |b| of the widest class
        top = np.sort(z, 1)
        knife = top[:, -1] - top[:, -2] < bound
        assert knife.mean() <= 0.05, (f, knife.mean())
        assert np.array_equal(pred[f][rows][~knife], z.argmax(1)[~knife]) and (pred[f][~rows] == -1).all()
        assert held[f] == rows.sum() and correct[f] == (pred[f][rows] == labels[rows]).sum()

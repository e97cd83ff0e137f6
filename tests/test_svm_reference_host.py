"""CPU: the numpy restatement of the finetune solver's Newton iteration (tests/svm_reference.py), which tests/test_gpu_svm_steps.py
holds the kernels of csrc/kernels_svm.hip to.  Nothing here runs a kernel.

  * The fp64 restatement, iterated to the stop test, is pinned to something independent: the fp64 optima of the golden fixtures
    (LinearSVC polished by exact Newton steps, tests/golden/make_golden_finetune.py), within the bound of
    test_gpu_finetune.test_solver_reaches_the_fp64_optimum.
  * The tolerances of the GPU tests are MEASURED here: the fp32-storage restatement against the fp64 one from the same iterate,
    per case (svm_reference.SVM_DEV_*), and asserted to still hold.
  * The conditions the GPU tests rely on are asserted on the reference alone: on every problem of every case the first step (and
    the second at C <= 1) takes t = 1 and the same number of CG iterations in fp32 and in fp64; at most 20 % of a case's problems
    are left out of a step comparison for a thin decision margin; fp32 and fp64 take the same number of Newton iterations at C <= 1.
    A seed that violates one of these is replaced; the cap never moves.
"""
import functools
import os
import types

import numpy as np
import pytest

from tests import svm_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
IDS = [R.case_id(c) for c in R.CASES]


@pytest.mark.parametrize('name', ['tiny', 'pair', 'small'])
def test_fp64_restatement_reaches_the_golden_optimum(name):
    z = np.load(os.path.join(GOLDEN, 'finetune_%s.npz' % name))
    x, labels, fold_ids = z['X'], z['labels'], z['fold_ids']
    d1 = x.shape[1] + 1
    cs = list(z['Cs'])
    worst, iters = 0.0, 0
    for p, (fold, cls, c) in enumerate(zip(z['prob_fold'], z['prob_class'], z['prob_C'])):
        if fold < 0:
            continue
        xt, y, c32 = R.problem(x, labels, fold_ids, fold, cls, c)
        sol = R.solve(xt, y, c32, eps=1e-5)
        assert sol.converged, (name, p, sol.iterations, sol.ratios[-1])
        held = fold_ids == fold
        xh = np.concatenate([x[held].astype(np.float64), np.ones((int(held.sum()), 1))], 1)
        err = np.abs(xh @ sol.w - xh @ z['w_star'][p])
        bound = 2.0 * z['dz_ref'][int(np.argmin(np.abs(np.array(cs) - c)))] + d1 * 2.0 ** -24 * (np.abs(xh) @ np.abs(z['w_star'][p]))
        worst, iters = max(worst, (err / bound).max()), max(iters, sol.iterations)
        assert (err <= bound).all(), (name, p, fold, c, err.max(), bound.min())
    print('%s: iterations <= %d, |z - z*| / bound <= %.3f' % (name, iters, worst))


@functools.lru_cache(maxsize=None)
def analyse(case):
    """Per problem of a case: the two restatements side by side, from the same iterates."""
    cd = R.case_data(case)
    s64, s32 = R.case_solutions(case, 'f64'), R.case_solutions(case, 'f32')
    rows = []
    for (xt, y, c), a, b in zip(cd.problems, s64, s32):
        g0 = float(np.linalg.norm(R.gradient(np.zeros(xt.shape[1]), xt, y, c)))
        r = types.SimpleNamespace(c=c, it64=a.iterations, it32=b.iterations, conv=a.converged and b.converged)
        a1, b1 = a.steps[0], b.steps[0]
        r.agree1 = a1.t == 1.0 and b1.t == 1.0 and a1.cg_iters == b1.cg_iters
        r.thin1 = a1.cg_margin < R.MARGIN
        r.dev1 = float(np.abs(a1.w_next - b1.w_next).max() / np.abs(a1.w_next).max())
        r.agree2, r.thin2, r.dev2 = True, False, 0.0
        if c <= 1.0 and len(b.steps) > 1:
            w1, b2 = b.iterates[1], b.steps[1]
            a2 = R.newton_step(w1, xt, y, c, g0)
            r.agree2 = a2.t == 1.0 and b2.t == 1.0 and a2.cg_iters == b2.cg_iters
            r.thin2 = R.thin(a2)
            r.dev2 = float(np.abs(a2.w_next - b2.w_next).max() / np.abs(a2.w_next - w1).max())
        r.dev_ratio = max(abs(rt - float(np.linalg.norm(R.gradient(w, xt, y, c))) / g0) for w, rt in zip(b.iterates, b.ratios))
        rows.append(r)
    return rows


def summary(case):
    rows = analyse(case)
    low = [r for r in rows if r.c <= 1.0]
    high = [r for r in rows if r.c > 1.0]
    return types.SimpleNamespace(
        dev1=max(r.dev1 for r in rows), dev2=max([r.dev2 for r in low if not r.thin2] or [0.0]),
        dev_ratio=max(r.dev_ratio for r in rows), thin1=np.mean([r.thin1 for r in rows]), thin2=np.mean([r.thin2 for r in low]),
        agree1=all(r.agree1 for r in rows), agree2=all(r.agree2 for r in low), same_low=all(r.it64 == r.it32 for r in low),
        gap_high=max([abs(r.it64 - r.it32) for r in high] or [0]), it64=max(r.it64 for r in rows), it32=max(r.it32 for r in rows),
        converged=all(r.conv for r in rows))


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_fp32_deviations_are_what_the_gpu_tolerances_assume(case):
    s = summary(case)
    print('%s: step 1 %.3g, step 2 %.3g, grad_ratio %.3g, Newton iterations fp64 <= %d, fp32 <= %d, apart at C = 100 <= %d'
          % (R.case_id(case), s.dev1, s.dev2, s.dev_ratio, s.it64, s.it32, s.gap_high))
    assert s.dev1 <= R.SVM_DEV_STEP1
    assert s.dev2 <= R.SVM_DEV_STEP2
    assert s.dev_ratio <= R.SVM_DEV_RATIO
    assert s.gap_high <= R.SVM_ITER_GAP_C100


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_the_conditions_the_gpu_tests_rely_on(case):
    s = summary(case)
    print('%s: left out of step 1 %.3f, of step 2 %.3f' % (R.case_id(case), s.thin1, s.thin2))
    assert s.converged
    assert s.agree1, 'first step: t = 1 and equal CG counts on every problem'
    assert s.agree2, 'second step at C <= 1: t = 1 and equal CG counts on every problem'
    assert s.thin1 <= R.EXCLUDED_CAP and s.thin2 <= R.EXCLUDED_CAP
    assert s.same_low, 'fp32 and fp64 Newton iteration counts at C <= 1'


def test_the_case_list_covers_the_edges_it_names():
    ps = {c[2] for c in R.CASES}
    assert {1, 63, 64, 65, 129, 54} <= ps
    assert {(c[0], c[1]) for c in R.CASES} == {(37, 1), (64, 2), (65, 31), (129, 32), (257, 63), (193, 64), (130, 255), (257, 256),
                                              (131, 280)}
    for case in R.CASES:
        cd = R.case_data(case)
        assert len(cd.cs) == case[2] and cd.x.dtype == np.float32 and cd.x.shape == case[:2] and (cd.x >= 0).all()
        assert ((cd.cs[54:] > 0.01) & (cd.cs[54:] < 1.0)).all()
        if case[2] >= 54:
            assert cd.cs[:3].tolist() == [0.01, 1.0, 100.0] and cd.folds[:54:9].tolist() == [-1, 0, 1, 2, 3, 4]


def test_restatement_degenerate_problems():
    # no training row: the gradient at 0 is 0, the ratio is defined as 0 and the stop test holds at once
    sol = R.solve(np.zeros((0, 3)), np.zeros(0), 1.0)
    assert sol.converged and sol.iterations == 0 and sol.ratios == [0.0] and not sol.w.any()
    # one class only: the minimiser has y z <= 1 everywhere and the threshold uses max(min(#pos, #neg), 1) = 1
    rng = np.random.default_rng(0)
    xt = np.concatenate([np.abs(rng.standard_normal((20, 2))), np.ones((20, 1))], 1)
    y = -np.ones(20)
    sol = R.solve(xt, y, 1.0)
    assert sol.converged and sol.ratios[-1] <= 1e-5 / 20
    assert R.stop_threshold(y, 1e-5, 2.0) == 1e-5 / 20 * 2.0

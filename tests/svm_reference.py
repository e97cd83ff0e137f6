"""The Newton iteration of the finetune solver (csrc/kernels_svm.hip, csrc/svm_api.hip) restated in plain numpy, one problem at a
time, and the case list of tests/test_svm_reference_host.py and tests/test_gpu_svm_steps.py.  numpy only: no torch, no package.

A problem is (xt, y, c): the TRAINING rows of X~ = [X, 1] in fp64, their targets +-1, and C as the device reads it (the table
stores C in fp32).  `newton_step` follows the kernels' rules, not liblinear's:

  k_svm_product<GRAD>, k_svm_newton_begin   z = X~ w;  A = {y z < 1} (strict);  g = w + 2C X~^T (A o (z - y));  |g|, the ratio
                                            |g| / |g(0)|, the stop test |g| <= eps max(min(#pos, #neg), 1) / max(n, 1) |g(0)|
  k_svm_product<HV>, k_svm_cg_step          s = 0, r = d = -g;  Hd = d + 2C X~^T (A o X~ d) with the A of this iteration;  stops at
                                            rr <= min(0.1, sqrt(|g| / |g0|))^2 |g|^2, after min(D + 1, 48) iterations, or at d.Hd <= 0
  k_svm_product<XS>, k_svm_ls_partial,      t = 1, 1/2, ..., 2^-11: the first with
  k_svm_newton_end                          t w.s + t^2/2 s.s + C sum(h(t)^2 - h(0)^2) <= 0.01 t g.s, provided g.s < 0;  w += t s;
                                            no such t: the problem ends NOT converged

`storage=np.float64` is the reference.  `storage=np.float32` rounds what the kernels keep in fp32 -- z, X~ d, X~ s, the
coefficients, the partial products of each 64-row slab, g, s, r, d, w -- and leaves the scalars in fp64, as on the device.  It only
serves to MEASURE how far correct fp32 arithmetic lies from fp64 (SVM_DEV_* below); nothing here comes from a kernel's output.
tests/test_svm_reference_host.py pins the fp64 restatement to the golden fp64 optima.
"""
import functools
import types

import numpy as np

CG_MAX = 48                # svm_api.hip SVM_CG_MAX
LS_NC = 12                 # kernels_svm.hip LS_NC: step lengths 1 ... 2^-11
SLAB = 64                  # kernels_svm.hip RS: rows per partial product
ARMIJO = 0.01
MARGIN = 0.02              # a decision closer than this to its threshold is "thin": the problem is left out of a step comparison
EXCLUDED_CAP = 0.20        # at most this share of a case's problems may be left out, per step
DEFAULT_EPS = 1e-5         # finetune.DEFAULT_EPS
DEFAULT_MAX_ITER = 100     # finetune.DEFAULT_MAX_ITER


def _xt_products(xt, storage):
    """(v -> X~ v, coef -> X~^T coef) with the roundings of `storage`: a product per row, one partial per 64-row slab."""
    if storage == np.float64:
        return (lambda v: xt @ v), (lambda coef: xt.T @ coef)
    n, d1 = xt.shape
    slabs = (n + SLAB - 1) // SLAB
    pad = np.zeros((slabs * SLAB, d1))
    pad[:n] = xt
    pad = pad.reshape(slabs, SLAB, d1)

    def forward(v):
        return (xt @ v).astype(np.float32).astype(np.float64)

    def backward(coef):
        c = np.zeros(slabs * SLAB)
        c[:n] = coef
        part = np.einsum('sr,srm->sm', c.reshape(slabs, SLAB), pad)
        return part.astype(np.float32).astype(np.float64).sum(0)
    return forward, backward


def objective(w, xt, y, c):
    h = np.maximum(0.0, 1.0 - y * (xt @ w))
    return 0.5 * (w @ w) + c * (h @ h)


def gradient(w, xt, y, c):
    """fp64 gradient of f at w, the active set strict as in the kernels."""
    z = xt @ w
    a = y * z < 1.0
    return w + 2.0 * c * (xt[a].T @ (z[a] - y[a]))


def stop_threshold(y, eps, g0norm):
    n = len(y)
    pos = int((y > 0).sum())
    return eps * max(min(pos, n - pos), 1) / max(n, 1) * g0norm


def newton_step(w, xt, y, c, g0norm, storage=np.float64, eps=None):
    """One Newton iteration from `w` (fp64 array holding values of `storage`).  `g0norm` is |g(0)| of the problem (None: `w` is
    the start and |g(w)| is taken).  Returns a namespace:

      g, gnorm, ratio       gradient at w, its norm, gnorm / g0norm (0 when g0norm is 0)
      stop                  the stop test holds at w (only with `eps`); no step is taken then and `w_next` is w
      cg_iters, t           CG iterations taken, accepted step length (0.0: the line search found none, `w_next` is w)
      s, w_next             the CG direction and w + t s
      cg_margin             smallest |ln(rr_j / cg_tol^2)| over the CG iterations before the last (inf when there is none)
      armijo_margin         smallest |df - 0.01 t g.s| / |0.01 t g.s| over the Armijo tests that were evaluated
      active_margin         smallest |1 - y z| on the training rows (inf without rows)
      active_margin_fp32    smallest |1 - y z| / ((D + 1) 2^-24 |x~|.|w|): the distance of a row from the edge of the active set in
                            units of the rounding bound of its fp32 dot product (see `thin`)
    """
    F = lambda a: np.asarray(a, np.float64) if storage == np.float64 else np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    forward, backward = _xt_products(xt, storage)
    w = np.asarray(w, np.float64)
    d1 = len(w)
    c2 = 2.0 * c
    z = forward(w)
    active = y * z < 1.0
    g = F(w + c2 * backward(np.where(active, F(z - y), 0.0)))
    gg = float(g @ g)
    gnorm = np.sqrt(gg)
    if g0norm is None:
        g0norm = gnorm
    ratio = gnorm / g0norm if g0norm > 0.0 else 0.0
    out = types.SimpleNamespace(g=g, gnorm=gnorm, ratio=ratio, g0norm=g0norm, stop=False, cg_iters=0, t=0.0, s=np.zeros(d1), w_next=w,
                                cg_margin=np.inf, armijo_margin=np.inf,
                                active_margin=float(np.abs(1.0 - y * z).min()) if len(y) else np.inf, active_margin_fp32=np.inf)
    if len(y):
        bound = d1 * 2.0 ** -24 * (np.abs(xt) @ np.abs(w))
        with np.errstate(divide='ignore'):
            out.active_margin_fp32 = float((np.abs(1.0 - y * z) / bound).min())
    if eps is not None and gnorm <= stop_threshold(y, eps, g0norm):
        out.stop = True
        return out

    rel = min(np.sqrt(ratio), 0.1)
    tol2 = rel * rel * gg
    cg_max = min(d1, CG_MAX)
    s, r, d = np.zeros(d1), -g, -g
    rr = gg
    logs = []
    while out.cg_iters < cg_max:
        hd = d + c2 * backward(np.where(active, forward(d), 0.0))
        dhd = float(d @ hd)
        if not dhd > 0.0:
            break
        alpha = rr / dhd
        s = F(s + alpha * d)
        r = F(r - alpha * hd)
        rr_new = float(r @ r)
        d = F(r + (rr_new / rr) * d)
        rr = rr_new
        out.cg_iters += 1
        with np.errstate(divide='ignore'):
            logs.append(abs(np.log(rr / tol2)) if tol2 > 0.0 else np.inf)
        if rr <= tol2:
            break
    if len(logs) > 1:
        out.cg_margin = float(min(logs[:-1]))
    out.s = s

    u = forward(s)
    m0 = 1.0 - y * z
    yu = y * u
    h0 = np.maximum(m0, 0.0) ** 2
    ws, ss, gs = float(w @ s), float(s @ s), float(g @ s)
    t = 1.0
    for _ in range(LS_NC):
        dl = float((np.maximum(m0 - t * yu, 0.0) ** 2 - h0).sum())
        df = t * ws + 0.5 * t * t * ss + c * dl
        if gs < 0.0:
            out.armijo_margin = min(out.armijo_margin, abs(df - ARMIJO * t * gs) / abs(ARMIJO * t * gs))
            if df <= ARMIJO * t * gs:
                out.t = t
                break
        t *= 0.5
    if out.t > 0.0:
        out.w_next = F(w + out.t * s)
    return out


def thin(step):
    """A decision of this step is too close to its threshold for two correct fp32 implementations to agree on it.

    The CG and Armijo margins are relative distances and are held to MARGIN.  The active-set margin |1 - y z| is an absolute
    distance in units of z: held to MARGIN it would leave out every problem at C = 1 (a few hundred rows spread over a margin of
    order one always put one within 0.02 of the edge), far beyond EXCLUDED_CAP.  What can move a row across the edge is the rounding
    of its fp32 dot product, at most (D + 1) 2^-24 |x~|.|w| in any summation order, so a row is on the knife edge when |1 - y z| is
    below TWICE that bound -- the rule of the scoring kernel's continuous case."""
    return min(step.cg_margin, step.armijo_margin) < MARGIN or step.active_margin_fp32 < 2.0


def solve(xt, y, c, eps=DEFAULT_EPS, max_iter=DEFAULT_MAX_ITER, storage=np.float64):
    """`newton_step` to the stop test, as fit_chunk runs it.  Returns a namespace with `iterates` (w_0 = 0, w_1, ...), `ratios`
    (|g(w_k)| / |g(0)| at each iterate), `steps` (the namespaces of the steps taken), `iterations` and `converged`."""
    w = np.zeros(xt.shape[1])
    out = types.SimpleNamespace(iterates=[w], ratios=[], steps=[], iterations=0, converged=False)
    g0norm = None
    while True:
        st = newton_step(w, xt, y, c, g0norm, storage, eps=eps)
        g0norm = st.g0norm
        out.ratios.append(st.ratio)
        if st.stop:
            out.converged = True
            break
        if out.iterations >= max_iter or st.t == 0.0:
            break
        out.steps.append(st)
        out.iterations += 1
        w = st.w_next
        out.iterates.append(w)
    out.w = w
    return out


# ----------------------------------------------------------------------------------------------------------------------
# The cases.  Data as tests/golden/make_golden_finetune.py makes them: features max(mu[y] + N(0, 1), 0) * 0.25 with
# mu = sep N(0, 1) per class, labels a permutation of arange(N) % K.  Row folds are arange(N) % 5; the table is
# (fold -1, 0..4) x (class 0..2) x (C 0.01, 1, 100) with C fastest: 54 problems.  P below 54 truncates the table; P above 54 extends
# it with further problems whose C lies inside (0.01, 1), folds and classes cycling.
# ----------------------------------------------------------------------------------------------------------------------
SEP = 0.5
CLASSES = 3
FOLDS = (-1, 0, 1, 2, 3, 4)
CS = (0.01, 1.0, 100.0)

# (N, D, P, seed): what the shape is there for
CASES = (
    (37, 1, 63, 11),        # one ragged slab, D + 1 = 2; one problem short of a tile
    (64, 2, 54, 22),        # one exact slab, odd D + 1 (padded to 4)
    (65, 31, 54, 13),       # second slab of one row, one exact column tile
    (65, 31, 1, 13),        # the same data, a single problem
    (129, 32, 64, 14),      # second column tile of one column; one exact problem tile
    (257, 63, 65, 15),      # second line-search group of one row; second problem tile of one problem
    (193, 64, 129, 56),     # D + 1 = 65; third problem tile of one problem
    (130, 255, 54, 37),
    (257, 256, 54, 68),
    (131, 280, 54, 149),     # the maximum width
)


def case_id(case):
    return 'n%d-d%d-p%d' % case[:3]


def make_data(n, d, k, sep, seed):
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.arange(n) % k).astype(np.int64)
    mu = sep * rng.standard_normal((k, d))
    x = np.maximum(mu[labels] + rng.standard_normal((n, d)), 0.0) * 0.25
    return x.astype(np.float32), labels


def make_table(p):
    """(folds, classes, Cs) of the first p problems."""
    rows = [(f, k, c) for f in FOLDS for k in range(CLASSES) for c in CS]
    extra = max(p - len(rows), 0)
    for j, c in enumerate(np.geomspace(0.01, 1.0, extra + 2)[1:-1]):
        rows.append((FOLDS[j % len(FOLDS)], (j // len(FOLDS)) % CLASSES, float(c)))
    rows = rows[:p]
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32),
            np.array([r[2] for r in rows], np.float64))


def problem(x, labels, row_fold, fold, cls, c):
    """(xt, y, c) of one table row: the training rows in fp64, and C as the fp32 table holds it."""
    train = row_fold != fold
    xt = np.concatenate([x[train].astype(np.float64), np.ones((int(train.sum()), 1))], 1)
    return xt, np.where(labels[train] == cls, 1.0, -1.0), float(np.float32(c))


@functools.lru_cache(maxsize=None)
def case_data(case):
    n, d, p, seed = case
    x, labels = make_data(n, d, CLASSES, SEP, seed)
    row_fold = (np.arange(n) % 5).astype(np.int32)
    folds, classes, cs = make_table(p)
    return types.SimpleNamespace(n=n, d=d, p=p, x=x, labels=labels, row_fold=row_fold, folds=folds, classes=classes, cs=cs,
                                 problems=[problem(x, labels, row_fold, f, k, c) for f, k, c in zip(folds, classes, cs)])


@functools.lru_cache(maxsize=None)
def case_solutions(case, storage_name):
    """`solve` of every problem of a case at the default eps, once per session: 'f64' or 'f32'."""
    storage = {'f64': np.float64, 'f32': np.float32}[storage_name]
    return [solve(xt, y, c, storage=storage) for xt, y, c in case_data(case).problems]


# Largest deviation of the fp32-storage restatement from the fp64 one FROM THE SAME ITERATE over the cases above, measured by
# tests/test_svm_reference_host.py, which asserts that they still hold: what correct fp32 arithmetic costs.  The kernels sum in
# another order (32 x 32 x 2 matrix steps, partials per row group), so they get 8 x these (tests/test_gpu_svm_steps.py).
SVM_DEV_STEP1 = 7e-6  # measured 6.44e-6:     # |w_1(fp32) - w_1(fp64)| / max|w_1|
SVM_DEV_STEP2 = 1.1e-3  # measured 1.00e-3:     # |w_2(fp32) - w_2(fp64)| / max|w_2 - w_1| from the fp32 w_1, at C <= 1
SVM_DEV_RATIO = 1e-7  # measured 9.76e-8:     # |grad_ratio(fp32) - fp64 |g(w_k)| / |g(0)|| at the iterates w_k of the fp32 trajectory, absolute
SVM_ITER_GAP_C100 = 5  # measured 5:   # largest |iterations(fp32) - iterations(fp64)| at C = 100

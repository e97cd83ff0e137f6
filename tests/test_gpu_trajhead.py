"""GPU: the head of a whole trajectory [T, N, C, H, W] in one call (tests/trajhead_cases.py has the cases and the fp64 references).

1. GroupNorm head: `FCClassifier.forward` on the trajectory is the loop over its slices bit for bit (no kernel of its own: the head's
   nodes on the flattened view), pooled within 1e-5 of max|ref| of the fp64 module sequence.
2. BatchNorm head: `bn_head_pool_slices` (node_bnhead_fwd_slices) is T calls of `bn_head_pool` bit for bit, statistics included.
3. Sliced loss: `node_head_loss_slices_fwd` is T calls of `node_head_loss_fwd(NODE_REDUCE_SUM)` bit for bit.
4. Distance: `trajectory_distance` (node_gn_relu_distance) against fp64, its error at most 4 x that of the fp32 chain of tensor
   operations `attack diff` ran before, which the test runs on the same inputs on the GPU.
5. End to end: nets, `evaluate accuracy`, `attack diff`.

Measured on an MI355X (every run prints its figures, `-s`): see the docstrings of the tests."""
import csv
import ctypes as C
import os

import pytest
import torch

from tests import trajhead_cases as K

pytestmark = pytest.mark.gpu


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


class _switch:
    """`FCClassifier.fused_trajectory` off inside the block"""

    def __enter__(self):
        import neural_ode_features_amd as nof
        nof.FCClassifier.fused_trajectory = False

    def __exit__(self, *exc):
        import neural_ode_features_amd as nof
        nof.FCClassifier.fused_trajectory = True


class _count:
    """counts the calls of the head's entry points (the functions `FCClassifier` reaches the library through) inside the block"""
    NAMES = ('head_pool', 'bn_head_pool', 'bn_head_pool_slices')

    def __enter__(self):
        from neural_ode_features_amd import head
        self.calls, self.saved = {k: 0 for k in self.NAMES}, {k: getattr(head, k) for k in self.NAMES}
        for k, fn in self.saved.items():
            def wrapped(*a, _k=k, _fn=fn, **kw):
                self.calls[_k] += 1
                return _fn(*a, **kw)
            setattr(head, k, wrapped)
        return self

    def __exit__(self, *exc):
        from neural_ode_features_amd import head
        for k, fn in self.saved.items():
            setattr(head, k, fn)

    @property
    def total(self):
        return sum(self.calls.values())


# ---------------------------------------------------------------------------------------------------------------------
# 1. GroupNorm head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out', K.GN_HEAD_OUTS, ids=['linear10', 'linear200', 'pool_only'])
@pytest.mark.parametrize('case', K.GN_HEAD_CASES, ids=str)
def test_group_norm_head_of_a_trajectory_is_the_loop_bit_for_bit(case, out):
    """pooled against fp64 on an MI355X: 1.3e-7 / 1.8e-7 / 9.8e-8 of max|ref| at the three shapes (bound 1e-5)."""
    T, n, c = case[:3]
    head = K.classifier(c, out, seed=K.seed_of(case)).cuda()
    x = K.trajectory(case).cuda()
    with torch.no_grad():
        with _count() as fused:
            got = head(x)
        with _switch(), _count() as loop:
            want = head(x)
        assert fused.calls['head_pool'] == 1 and loop.calls['head_pool'] == T
        assert got.shape == (T, n, out if out else c) and torch.equal(got, want)
        assert torch.equal(got, torch.stack([head(xi) for xi in x]))
        pooled = head.pooled(x.reshape(T * n, *case[2:])).reshape(T, n, c)
    err = _rel(pooled, K.pooled_fp64(head, x))
    print('trajhead gn %s out=%s: pooled max error / max|ref| = %.2e (bound %.0e)' % (case, out, err, K.POOLED_FLOOR))
    assert err <= K.POOLED_FLOOR


def test_group_norm_head_of_a_trajectory_stays_differentiable():
    """a view plus the existing nodes: the gradients of the one call are those of the loop (sums of T terms in another order)"""
    case = (3, 2, 64, 8, 8)
    head = K.classifier(64, 10, seed=5).cuda()
    x = K.trajectory(case).cuda().requires_grad_(True)
    cot = torch.randn(3, 2, 10, generator=torch.Generator().manual_seed(6)).cuda()
    ps = [x] + list(head.parameters())
    g_one = torch.autograd.grad(head(x), ps, cot)
    with _switch():
        g_loop = torch.autograd.grad(head(x), ps, cot)
    assert torch.equal(g_one[0], g_loop[0])                                       # dz: per sample
    for a, b in zip(g_one[1:], g_loop[1:]):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 2. BatchNorm head, sliced
# ---------------------------------------------------------------------------------------------------------------------
def _bn_check(case, x):
    from neural_ode_features_amd import _lib, head as H
    T, n, c, h, w = case
    clf = K.classifier(c, None, norm='batch', seed=K.seed_of(case)).cuda()
    bn = clf.module[0]
    x = x.cuda()
    lib = _lib.load()
    with torch.no_grad():
        assert H.bn_head_slices_fusable(x, bn)
        got = H.bn_head_pool_slices(x, bn.weight, bn.bias, bn.eps)
        want = torch.stack([H.bn_head_pool(xi, bn.weight, bn.bias, bn.eps) for xi in x])
        assert torch.equal(got, want)
        # the statistics, straight from the two entry points
        shape = _lib.NodeBnfuncShape(n, c, h, w, bn.eps)
        st = torch.empty(T, 2, c, device='cuda')
        pooled = torch.empty(T, n, c, device='cuda')
        scratch = torch.empty(lib.node_bnhead_slices_scratch_bytes(shape, T) // 8, device='cuda', dtype=torch.float64)
        _lib.check(lib.node_bnhead_fwd_slices(shape, T, x.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), pooled.data_ptr(),
                                              st.data_ptr(), scratch.data_ptr(), None))
        one = torch.empty(lib.node_bnhead_scratch_bytes(shape) // 8, device='cuda', dtype=torch.float64)
        for t in range(T):
            st1, p1 = torch.empty(2, c, device='cuda'), torch.empty(n, c, device='cuda')
            _lib.check(lib.node_bnhead_fwd(shape, x[t].data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), None, p1.data_ptr(),
                                           st1.data_ptr(), one.data_ptr(), None))
            assert torch.equal(st[t], st1) and torch.equal(pooled[t], p1), t
        assert torch.equal(pooled, got)
        with _count() as fused:
            out = clf(x)
        with _switch(), _count() as loop:
            assert torch.equal(out, clf(x))
        assert fused.calls == {'head_pool': 0, 'bn_head_pool': 0, 'bn_head_pool_slices': 1} and loop.calls['bn_head_pool'] == T
        assert torch.equal(out, got)
    err = _rel(got, K.pooled_fp64(clf, x))
    print('trajhead bn %s: pooled max error / max|ref| = %.2e (bound %.0e)' % (case, err, K.POOLED_FLOOR))
    assert err <= K.POOLED_FLOOR


@pytest.mark.parametrize('case', K.BN_HEAD_CASES, ids=str)
def test_sliced_batch_norm_head_is_a_call_per_slice_bit_for_bit(case):
    """pooled against fp64 on an MI355X: 1.3e-7 / 1.5e-7 / 1.3e-7 / 1.1e-7 of max|ref| at the four shapes (bound 1e-5)."""
    _bn_check(case, K.trajectory(case))


def test_sliced_batch_norm_head_keeps_every_slice_its_own_statistics():
    """z = 50 + randn, slice s a further 10 s: 5.3e-6 of max|ref| on an MI355X (an fp32 input of size 50 to 70 carries 3e-6 to 4e-6
    of the spread in its own rounding; bound 1e-5).  Statistics shared between slices would be off by whole units."""
    _bn_check(K.BN_OFFSET_CASE, K.trajectory(K.BN_OFFSET_CASE, offset=50.0, slice_shift=10.0))


def test_sliced_batch_norm_head_is_refused_where_a_backward_may_follow():
    from neural_ode_features_amd import head as H
    clf = K.classifier(64, 10, norm='batch').cuda()
    x = K.trajectory((3, 2, 64, 8, 8)).cuda()
    assert not H.bn_head_slices_fusable(x, clf.module[0])                         # parameters that want gradients, grad mode on
    with _count() as calls:
        out = clf(x)
    assert calls.calls['bn_head_pool'] == 3 and calls.calls['bn_head_pool_slices'] == 0 and out.requires_grad
    with torch.no_grad():
        assert H.bn_head_slices_fusable(x, clf.module[0])
        assert not H.bn_head_slices_fusable(x.transpose(0, 1), clf.module[0])     # not contiguous
        assert torch.equal(clf(x), out)


# ---------------------------------------------------------------------------------------------------------------------
# 3. sliced loss
# ---------------------------------------------------------------------------------------------------------------------
def _loss_slices(pooled, weight, bias, target, logits=None):
    """(logits, loss [T], stat [T, 2]) of node_head_loss_slices_fwd: from pooled, or from given logits"""
    from neural_ode_features_amd import _lib, head as H
    lib = _lib.load()
    T, n = (pooled if logits is None else logits).shape[:2]
    o = weight.shape[0]
    lg = torch.empty(T, n, o, device='cuda') if logits is None else logits
    loss, stat = torch.full((T,), -1.0, device='cuda'), torch.full((T, 2), -1.0, device='cuda')
    scratch = H._slices_scratch(lg.device, T, n)
    if logits is None:
        h = _lib.NodeHeadLossSlices(T, n, pooled.shape[2], o, pooled.data_ptr(), weight.data_ptr(), bias.data_ptr(), target.data_ptr(),
                                    lg.data_ptr(), loss.data_ptr(), stat.data_ptr(), scratch.data_ptr())
    else:
        h = _lib.NodeHeadLossSlices(T, n, 0, o, None, None, None, target.data_ptr(), lg.data_ptr(), loss.data_ptr(), stat.data_ptr(),
                                    scratch.data_ptr())
    _lib.check(lib.node_head_loss_slices_fwd(C.byref(h), None))
    return lg, loss, stat


def _loss_one(pooled, weight, bias, target, logits=None):
    """the same of node_head_loss_fwd(NODE_REDUCE_SUM) on one slice"""
    from neural_ode_features_amd import _lib, head as H
    lib = _lib.load()
    n = (pooled if logits is None else logits).shape[0]
    o = weight.shape[0]
    lg = torch.empty(n, o, device='cuda') if logits is None else logits
    loss, stat = torch.empty((), device='cuda'), torch.empty(2, device='cuda')
    h = H._loss_struct(n, pooled.shape[1] if logits is None else 0, o, _lib.REDUCE_SUM, pooled=pooled if logits is None else None,
                       weight=weight if logits is None else None, bias=bias if logits is None else None, target=target, logits=lg,
                       loss=loss, stat=stat, scratch=H._scratch(lg.device, n))
    _lib.check(lib.node_head_loss_fwd(C.byref(h), None))
    return lg, loss, stat


@pytest.mark.parametrize('given', [False, True], ids=['from_pooled', 'logits_given'])
@pytest.mark.parametrize('case', K.LOSS_CASES, ids=str)
def test_sliced_loss_is_a_launch_per_slice_bit_for_bit(case, given):
    import neural_ode_features_amd as nof
    T, n, c, o = case
    pooled, weight, bias, target = (t.cuda() for t in K.loss_inputs(case))
    logits = (pooled @ weight.t() + bias).contiguous() if given else None
    lg, loss, stat = _loss_slices(pooled, weight, bias, target, logits)
    for t in range(T):
        lg1, loss1, stat1 = _loss_one(pooled[t], weight, bias, target, None if logits is None else logits[t])
        assert torch.equal(lg[t], lg1), t
        assert torch.equal(loss[t], loss1) and torch.equal(stat[t], stat1), (t, loss[t], loss1, stat[t], stat1)
    assert torch.equal(stat[:, 0], loss)
    assert torch.equal(stat[:, 1], (lg.argmax(-1) == target).sum(-1).float())
    lg2, loss2, stat2 = _loss_slices(pooled, weight, bias, target, logits)              # two runs, the same bits
    assert torch.equal(lg2, lg) and torch.equal(loss2, loss) and torch.equal(stat2, stat)
    # the public function, and the same quantities in fp64
    pub = nof.trajectory_loss(lg, target)
    assert torch.equal(pub, stat)
    ref_loss, ref_hits = K.loss_fp64(lg, target)
    assert torch.equal(stat[:, 1].cpu().double(), ref_hits)
    assert float((stat[:, 0].cpu().double() - ref_loss).abs().max()) <= 1e-5 * max(1.0, float(ref_loss.abs().max()))
    # ... and what `cross_entropy(reduction='sum')` returns for a slice
    ce = nof.cross_entropy(lg[0], target, reduction='sum')
    assert torch.equal(ce, stat[0, 0]) and torch.equal(ce.node_stat, stat[0])


def test_sliced_loss_scratch_serves_another_batch_size_and_stays_zeroed():
    from neural_ode_features_amd import head as H
    import neural_ode_features_amd as nof
    gen = torch.Generator().manual_seed(9)
    for n in (7, 3, 12):
        lg = torch.randn(5, n, 10, generator=gen).cuda()
        tg = torch.randint(0, 10, (n,), generator=gen).cuda()
        stat = nof.trajectory_loss(lg, tg)
        want = torch.stack([nof.cross_entropy(lg[t], tg, reduction='sum').node_stat for t in range(5)])
        assert torch.equal(stat, want), n
        buf = H._slices_scratch(lg.device, 5, n)
        assert int(buf[:8].view(torch.int32).abs().sum()) == 0                          # the arrival counters are back at zero


# ---------------------------------------------------------------------------------------------------------------------
# 4. distance
# ---------------------------------------------------------------------------------------------------------------------
def _distance_errors(l2, cos, l2_64, cos_64):
    return float(((l2.cpu().double() - l2_64) / l2_64).abs().max()), float((cos.cpu().double() - cos_64).abs().max())


@pytest.mark.parametrize('case', K.DIST_CASES, ids=str)
def test_distance_against_fp64_within_four_times_the_tensor_chain(case):
    """Relative error of l2 / absolute error of cos against the fp64 module chain, kernel | the fp32 chain of tensor operations on
    the GPU (the bound is 4 x the chain's), measured on an MI355X:
        (3, 2, 64, 8, 8)    l2 6.7e-8 | 6.7e-8    cos 2.7e-8 | 6.2e-8
        (2, 3, 64, 7, 7)    l2 8.8e-8 | 6.9e-8    cos 1.6e-8 | 1.3e-7     (the one-thread-per-channel kernel)
        (5, 1, 256, 8, 8)   l2 7.0e-8 | 3.4e-8    cos 1.4e-8 | 7.4e-8
    All of them are the rounding of the fp32 result itself (half an ulp is 6e-8): the kernel adds its four sums in fp64."""
    import neural_ode_features_amd as nof
    traj0, traj1, norm, l2_64, cos_64 = K.distance_case(case)
    a, b, gn = traj0.cuda(), traj1.cuda(), K.group_norm(case[2], K.seed_of(case)).cuda()
    l2, cos = nof.trajectory_distance(a, b, gn)
    assert l2.shape == cos.shape == case[:2]
    k_l2, k_cos = _distance_errors(l2, cos, l2_64, cos_64)
    c_l2, c_cos = _distance_errors(*K.aten_distance(a, b, gn), l2_64, cos_64)
    print('trajhead distance %s: l2 rel error kernel %.2e | chain %.2e;  cos abs error kernel %.2e | chain %.2e' % (case, k_l2, c_l2, k_cos, c_cos))
    assert k_l2 <= 4 * c_l2 and k_cos <= 4 * c_cos
    l2b, cosb = nof.trajectory_distance(a, b, gn)                                       # two runs, the same bits
    assert torch.equal(l2, l2b) and torch.equal(cos, cosb)


@pytest.mark.parametrize('case', K.DIST_CASES, ids=str)
def test_distance_of_a_trajectory_to_itself_and_of_dead_features(case):
    import neural_ode_features_amd as nof
    a = K.trajectory(case).cuda()
    gn = K.group_norm(case[2], K.seed_of(case)).cuda()
    l2, cos = nof.trajectory_distance(a, a.clone(), gn)
    assert float(l2.abs().max()) == 0.0 and float((cos - 1).abs().max()) <= 1e-5
    with torch.no_grad():                 # beta = -8 with |gamma| <= 0.2: |xhat| <= sqrt(M - 1) < 40 for groups of M <= 1600 values
        gn.weight.clamp_(-0.2, 0.2)
        gn.bias.fill_(-8.0)
    b = a + 0.05 * torch.randn(*case, generator=torch.Generator().manual_seed(3)).cuda()
    l2, cos = nof.trajectory_distance(a, b, gn)
    assert bool(torch.isfinite(l2).all()) and bool(torch.isfinite(cos).all())
    assert float(l2.abs().max()) == 0.0 and float(cos.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', ['group', 'batch'])
def test_odenet_features_take_one_head_call_per_trajectory(norm):
    import neural_ode_features_amd as nof
    torch.manual_seed(0)
    net = nof.ODENet(1, n_filters=64, adjoint=True, norm=norm).cuda().eval()
    net.to_features_extractor()
    net.odeblock.t1 = [0.25, 0.5, 1]
    x = torch.rand(4, 1, 28, 28, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        with _count() as fused:
            on = net(x)
        with _switch(), _count() as loop:
            off = net(x)
    T = on.shape[0]
    assert on.shape == (T, 4, 64) and T >= 3 and torch.equal(on, off)
    assert fused.total == 1 and loop.total == T


def test_resnet_features_take_two_head_calls():
    import neural_ode_features_amd as nof
    torch.manual_seed(0)
    net = nof.ResNet(1, n_filters=64).cuda().eval()
    net.to_features_extractor()
    x = torch.rand(4, 1, 28, 28, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        with _count() as fused:
            on = net(x)
        with _switch(), _count() as loop:
            off = net(x)
    assert on.shape == (7, 4, 64) and torch.equal(on, off)
    assert fused.total == 2 and loop.total == 7


def test_unpooled_extractor_runs_the_norm_once_on_the_flattened_trajectory():
    import neural_ode_features_amd as nof
    from neural_ode_features_amd import head
    torch.manual_seed(0)
    net = nof.ODENet(1, n_filters=64, adjoint=True).cuda().eval()
    net.to_features_extractor(keep_pool=False)
    net.odeblock.t1 = [0.5, 1]
    x = torch.rand(2, 1, 28, 28, generator=torch.Generator().manual_seed(1)).cuda()
    calls, saved = [], head.gn_relu
    head.gn_relu = lambda z, norm, relu=True: (calls.append(tuple(z.shape)), saved(z, norm, relu))[1]
    try:
        with torch.no_grad():
            on = net(x)
    finally:
        head.gn_relu = saved
    T = on.shape[0]
    assert on.shape == (T, 2, 64, 7, 7) and T >= 3 and (T * 2, 64, 7, 7) in calls and (2, 64, 7, 7) not in calls
    with torch.no_grad():
        raw = net.odeblock(net.downsample(x))
        want = torch.stack([head.gn_relu(v, net.classifier[0]) for v in raw])
    assert torch.equal(on, want)


def _rows(path):
    with open(path) as fh:
        return list(csv.DictReader(fh))


def test_accuracy_sweep_with_the_sliced_loss_and_with_the_tensor_chain(tmp_path):
    from neural_ode_features_amd import evaluate as E
    from neural_ode_features_amd import train as T
    run = str(tmp_path / 'run')
    assert T.main(['--dataset', 'mnist', '-f', '16', '-b', '32', '--synthetic-size', '64', '-a', '--lr', '0.05', '-e', '1',
                   '--run-dir', run]) == 0
    argv = ['accuracy', run, '--t1', '0', '0.25', '0.5', '1', '--tol', '1e-3', '--limit', '32']
    new = _rows(E.main(argv))
    with _switch():
        old = _rows(E.main(argv))
    assert len(new) == len(old) == 4 and list(new[0]) == ['t1', 'test_loss', 'test_acc', 'test_nfe', 'test_tol']
    for a, b in zip(new, old):
        assert a['t1'] == b['t1'] and a['test_acc'] == b['test_acc'] and a['test_nfe'] == b['test_nfe'] and a['test_tol'] == b['test_tol']
        print('trajhead accuracy t1=%s: test_loss %s | %s' % (a['t1'], a['test_loss'], b['test_loss']))
        assert abs(float(a['test_loss']) - float(b['test_loss'])) <= 1e-6 * abs(float(b['test_loss']))


def test_attack_diff_with_the_distance_kernel_and_with_the_tensor_chain(tmp_path):
    """The two `diff` files of four attacked images, kernel against the chain of tensor operations on the same raw trajectories.
    Both are fp32 evaluations of one quantity, so they differ by at most the sum of their errors: (1 + 4) x the chain's error, with
    the chain's error of test 4 above (K.CHAIN_L2_REL, K.CHAIN_COS_ABS: its worst case there)."""
    from neural_ode_features_amd import attack as A
    from neural_ode_features_amd import train as T
    run, data = str(tmp_path / 'run'), str(tmp_path / 'data.pt')
    gen = torch.Generator().manual_seed(5)
    blob = dict(x_train=torch.randint(0, 256, (64, 1, 28, 28), generator=gen).to(torch.uint8), y_train=torch.arange(64) % 10,
                x_test=torch.randint(0, 256, (32, 1, 28, 28), generator=gen).to(torch.uint8), y_test=torch.zeros(32, dtype=torch.int64))
    torch.save(blob, data)
    assert T.main(['--dataset', 'mnist', '-f', '64', '-b', '32', '--data', data, '-a', '--lr', '0.001', '-e', '1', '-t', '1e-2',
                   '--augmentation', 'crop', '--run-dir', run]) == 0
    model, _ = A.load_run_raw(run)
    model = model.cuda().eval()
    model.odeblock.tol = 1e-2
    with torch.no_grad():
        blob['y_test'][:4] = model(A.unit_images(blob['x_test'][:4]).cuda()).argmax(1).cpu()
    torch.save(blob, data)
    argv = [run, '-t', '1e-2', '-e', '0.5', '-d', 'inf', '-s', '0.1', '--batch-size', '4', '--limit', '4']
    A.main(['attack'] + argv)
    seen = []
    from neural_ode_features_amd import head
    real = head.trajectory_distance
    head.trajectory_distance = lambda *a: (seen.append(tuple(a[0].shape)), real(*a))[1]
    try:
        l2_path, cos_path = A.main(['diff'] + argv + ['-r', '4'])
    finally:
        head.trajectory_distance = real
    assert seen == [(5, 4, 64, 7, 7)]                                # one call for the batch: raw trajectories of resolution + 1 slices
    new = _rows(l2_path), _rows(cos_path)
    assert new[0], 'no adversarial found: nothing to compare'
    os.remove(l2_path), os.remove(cos_path)
    with _switch():
        A.main(['diff'] + argv + ['-r', '4'])
    old = _rows(l2_path), _rows(cos_path)
    for k, (rows_new, rows_old) in enumerate(zip(new, old)):
        assert len(rows_new) == len(rows_old) and list(rows_new[0]) == list(rows_old[0])
        for a, b in zip(rows_new, rows_old):
            assert a['sample_id'] == b['sample_id']
            for col in list(a)[1:]:
                u, v = float(a[col]), float(b[col])
                print('trajhead diff %s sample %s t=%s: %.9g | %.9g' % ('l2' if k == 0 else 'cos', a['sample_id'], col, u, v))
                if k == 0:
                    assert abs(u - v) <= 5 * K.CHAIN_L2_REL * abs(v), (col, u, v)
                else:
                    assert abs(u - v) <= 5 * K.CHAIN_COS_ABS, (col, u, v)
